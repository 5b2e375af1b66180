#!/usr/bin/env python3
"""Generate golden vectors by IMPORTING the reference (read-only, in this container only).

Run:  python tests/golden/make_golden.py [--only NAME ...]

The reference lives at /root/reference and never travels to the GPU box, so what is
committed here is DATA only: inputs (FASTA, gz) and the reference's outputs for them
(.npz).  Nothing below copies reference source; the reference functions are called in
place (functions.get_orfs / functions.get_graph) and their local
variables are observed with sys.setprofile.

The shortest path is NOT computed by the reference's solver (fastpathz is an external
package absent from this container and from /root/reference — SURVEY.md §2 row 8), so the
path part of every fixture is produced by the exact-integer Bellman-Ford below, which
restates what phanotate.py:56-67 feeds to / reads from fastpathz: edges in
Graph.iteredges order, weight = trunc(Decimal_weight*1000) as an arbitrary-precision
int, in-place relaxation with strict '<', V-1 rounds with early exit.  It is cross-checked
against the only pinned results the reference repo holds (README.md:45-54, phiX174).
"""
import argparse
import ctypes
import gzip
import io
import os
import sys
import time
from decimal import Decimal

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
from phanotate_modules import functions  # noqa: E402  (the reference, imported in place)
from phanotate_modules.edges import Edge  # noqa: E402

D = Decimal


class StubLocus:
    """What functions.get_orfs needs from a genbank Locus (phanotate.py:42-44, orfs.py:8-15)."""

    def __init__(self, seq, start_codons="atg:0.85,gtg:0.10,ttg:0.05", stop_codons="tag,tga,taa", minlen=90):
        self._seq = seq
        sc = dict()
        for codon, weight in map(lambda x: tuple(x.split(":")), start_codons.split(",")):
            sc[codon.lower()] = D(weight)
        m = max(sc.values())
        self.start_codons = {k: v / m for k, v in sc.items()}  # file_handling.py:58-62
        self.stop_codons = [c.lower() for c in stop_codons.split(",")]
        self.min_orf_len = minlen

    def seq(self):
        return self._seq


def read_fasta(path):
    op = gzip.open if path.endswith(".gz") else open
    name, seq = None, []
    with op(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                if name is not None:
                    break
                name = line[1:].split()[0]
            else:
                seq.append(line.strip())
    return name, "".join(seq)


def run_reference(locus):
    """get_orfs + get_graph, capturing get_orfs' locals on return."""
    captured = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "get_orfs":
            loc = frame.f_locals
            for k in ("background_rbs", "training_rbs", "pos_max", "pos_min", "gc_pos_freq"):
                captured[k] = loc[k]

    t0 = time.time()
    sys.setprofile(prof)
    try:
        orfs = functions.get_orfs(locus)
    finally:
        sys.setprofile(None)
    t1 = time.time()
    graph = functions.get_graph(orfs)
    t2 = time.time()
    return orfs, graph, captured, (t1 - t0, t2 - t1)


def trunc_int(dec):
    """Decimal -> int, truncation toward zero (fastpathz drops the fractional digits)."""
    return int(dec)


def bellman_ford(nodes, edges, src, dst):
    """Exact-integer in-place Bellman-Ford over the edge list in the given order."""
    idx = {n: i for i, n in enumerate(nodes)}
    E = [(idx[e.source], idx[e.target], trunc_int(e.weight * 1000)) for e in edges]
    V = len(nodes)
    INF = None
    dist = [INF] * V
    par = [-1] * V
    dist[idx[src]] = 0
    rounds = 0
    for _ in range(V - 1):
        changed = False
        rounds += 1
        for (u, v, w) in E:
            du = dist[u]
            if du is None:
                continue
            nd = du + w
            if dist[v] is None or nd < dist[v]:
                dist[v] = nd
                par[v] = u
                changed = True
        if not changed:
            break
    t = idx[dst]
    if dist[t] is None:
        return [], None, rounds, E
    path = [t]
    while path[-1] != idx[src]:
        path.append(par[path[-1]])
    path.reverse()
    return path, dist[t], rounds, E


TYPE_CODE = {"start": 0, "stop": 1, "source": 2, "target": 3}


FAKE_ARAGORN = """#!/bin/sh
# stand-in for `aragorn -t -w <fasta>` while the fixtures are generated: prints the hit list of the case (batch format, -w)
printf '%s' "$PHX_FAKE_ARAGORN_OUT"
"""


def aragorn_text(trnas):
    """`aragorn -t -w` output for the hits [(begin, end, complement)]: what functions.add_trnas parses (functions.py:470-480)."""
    lines = [">temp", "%d genes found" % len(trnas)]
    for k, (a, b, c) in enumerate(trnas):
        lines.append("%-3d tRNA-Xxx %20s[%d,%d]      35      (nnn)" % (k + 1, "c" if c else "", a, b))
    return "\n".join(lines) + "\n"


def make_case(case, name, seq, outdir, trnas=None, **params):
    locus = StubLocus(seq, **params)
    out = {"name": name, "L": len(seq)}
    if trnas is not None:  # a fake `aragorn` on PATH (tRNAscan-SE stays absent): functions.py:457-509 runs as upstream would
        import tempfile

        td = tempfile.mkdtemp()
        exe = os.path.join(td, "aragorn")
        with open(exe, "w") as f:
            f.write(FAKE_ARAGORN)
        os.chmod(exe, 0o755)
        os.environ["PATH"] = td + os.pathsep + os.environ["PATH"]
        os.environ["PHX_FAKE_ARAGORN_OUT"] = aragorn_text(trnas)
        # the list add_trnas builds: [begin, end], reversed for a complement hit
        out["trna_start"] = np.array([b if c else a for a, b, c in trnas], dtype=np.int32)
        out["trna_stop"] = np.array([a if c else b for a, b, c in trnas], dtype=np.int32)
        out["aragorn_text"] = aragorn_text(trnas)
    out["params_start"] = ",".join("%s:%s" % (k, v) for k, v in locus.start_codons.items())
    out["params_stop"] = ",".join(locus.stop_codons)
    out["params_minlen"] = locus.min_orf_len
    if params:  # the flags as written (tests/test_params_gpu.py hands these to the product)
        out["flags_start"] = params.get("start_codons", "atg:0.85,gtg:0.10,ttg:0.05")
        out["flags_stop"] = params.get("stop_codons", "tag,tga,taa")
        # the suite reads params_start (conftest.golden_params): normalising that text once more must give the same dict
        again = StubLocus(seq, out["params_start"], out["params_stop"], locus.min_orf_len)
        assert list(again.start_codons.items()) == list(locus.start_codons.items()), (case, again.start_codons, locus.start_codons)
        assert again.stop_codons == locus.stop_codons
        assert all(len(str(v)) < 32 for v in locus.start_codons.values()), case  # libphx holds a weight's text in 31 characters
    try:
        try:
            orfs, graph, cap, times = run_reference(locus)
        finally:
            if trnas is not None:
                os.environ["PATH"] = os.pathsep.join(os.environ["PATH"].split(os.pathsep)[1:])
                os.environ.pop("PHX_FAKE_ARAGORN_OUT")
    except Exception as e:  # reference aborts the run: record which way
        out["error"] = type(e).__name__
        np.savez_compressed(os.path.join(outdir, case + ".npz"), **{k: np.array(v) for k, v in out.items()})
        print("%-22s L=%-7d reference raised %s" % (case, len(seq), out["error"]))
        return
    out["error"] = ""
    out["ref_seconds"] = np.array(times)
    out["pstop"] = float(orfs.pstop)
    out["pstop_str"] = str(orfs.pstop)
    out["background_rbs"] = np.array(cap["background_rbs"], dtype=np.float64)
    out["training_rbs"] = np.array(cap["training_rbs"], dtype=np.float64)
    out["pos_max"] = np.array([float(x) for x in cap["pos_max"]])
    out["pos_min"] = np.array([float(x) for x in cap["pos_min"]])
    out["gc_pos_freq"] = np.array(cap["gc_pos_freq"], dtype=np.int16)  # [L-1][3], row 0 is a dummy

    ol = list(orfs.iter_orfs())
    out["orf_start"] = np.array([o.start for o in ol], dtype=np.int32)
    out["orf_stop"] = np.array([o.stop for o in ol], dtype=np.int32)
    out["orf_frame"] = np.array([o.frame for o in ol], dtype=np.int32)
    out["orf_length"] = np.array([o.length for o in ol], dtype=np.int32)
    out["orf_rbs"] = np.array([o.rbs_score for o in ol], dtype=np.int32)
    out["orf_pstop"] = np.array([float(o.pstop) for o in ol])
    out["orf_weight_rbs"] = np.array([float(o.weight_rbs) for o in ol])
    out["orf_log10_hold"] = np.array([float(D(o.hold).log10()) if o.hold != 0 else -np.inf for o in ol])
    out["orf_weight"] = np.array([float(o.weight) for o in ol])
    out["orf_weight_str"] = np.array([str(o.weight) for o in ol])
    kt = sorted(int(k[1:]) for k in orfs.other_end if isinstance(k, str))  # 't'-prefixed keys of the tRNA nodes (functions.py:502-508)
    out["other_end_tkey"] = np.array(kt, dtype=np.int32)
    out["other_end_tval"] = np.array([orfs.other_end["t" + str(k)] for k in kt], dtype=np.int32)
    ks = sorted(k for k in orfs.other_end if isinstance(k, int))
    out["other_end_key"] = np.array(ks, dtype=np.int32)
    out["other_end_val"] = np.array([orfs.other_end[k] for k in ks], dtype=np.int32)

    nodes = list(graph.iternodes())
    nidx = {n: i for i, n in enumerate(nodes)}
    out["node_gene"] = np.array([n.gene for n in nodes])
    out["node_type"] = np.array([TYPE_CODE[n.type] for n in nodes], dtype=np.int8)
    out["node_frame"] = np.array([n.frame for n in nodes], dtype=np.int8)
    out["node_pos"] = np.array([n.position for n in nodes], dtype=np.int32)
    edges = list(graph.iteredges())
    out["edge_src"] = np.array([nidx[e.source] for e in edges], dtype=np.int32)
    out["edge_dst"] = np.array([nidx[e.target] for e in edges], dtype=np.int32)
    out["edge_weight"] = np.array([float(e.weight) for e in edges])
    import hashlib

    h = hashlib.md5()
    for e in edges:
        h.update((str(e) + "\n").encode())  # == the reference's --dump text (phanotate.py:58)
    out["dump_md5"] = h.hexdigest()

    src = nodes[-2] if len(nodes) >= 2 else None
    dst = nodes[-1] if len(nodes) >= 2 else None
    genes = []
    tab = io.StringIO()
    tab.write("#id:\t" + name + "\n")
    tab.write("#START\tSTOP\tFRAME\tCONTIG\tSCORE\n")
    if len(graph) > 2:  # phanotate.py:63
        path, dist, rounds, E = bellman_ford(nodes, edges, src, dst)
        out["edge_wint"] = np.array([str(w) for (_, _, w) in E])
        out["path"] = np.array(path, dtype=np.int32)
        out["path_dist"] = str(dist)
        out["bf_rounds"] = rounds
        sp = path[1:]  # phanotate.py:65
        it = iter(sp)
        for a, b in zip(it, it):  # file_handling.pairwise (phanotate.py:71)
            left, right = nodes[a], nodes[b]
            w = graph.weight(Edge(left, right, 0))
            strand = -1 if left.frame < 0 else 1
            l, r = left.position, right.position + 2  # locus.py:30
            genes.append((l, r, strand, float(w), left.frame))
            a_, b_ = (l, r) if strand > 0 else (r, l)  # locus.py:44-46
            if left.gene == "CDS":  # Locus.tabular prints features(include=['CDS']) only (locus.py:42)
                tab.write("%d\t%d\t%s\t%s\t%s\n" % (a_, b_, chr(44 - strand), name, "%E" % w))
    else:
        out["edge_wint"] = np.array([], dtype="U1")
        out["path"] = np.array([], dtype=np.int32)
        out["path_dist"] = ""
        out["bf_rounds"] = 0
    out["gene_left"] = np.array([g[0] for g in genes], dtype=np.int32)
    out["gene_right"] = np.array([g[1] for g in genes], dtype=np.int32)
    out["gene_strand"] = np.array([g[2] for g in genes], dtype=np.int8)
    out["gene_score"] = np.array([g[3] for g in genes])
    out["gene_frame"] = np.array([g[4] for g in genes], dtype=np.int8)
    out["tabular"] = tab.getvalue()
    np.savez_compressed(os.path.join(outdir, case + ".npz"), **{k: np.array(v) for k, v in out.items()})
    print(
        "%-22s L=%-7d orfs=%-5d nodes=%-5d edges=%-6d genes=%-4d rounds=%-3d ref get_orfs=%.2fs get_graph=%.2fs"
        % (case, len(seq), len(ol), len(nodes), len(edges), len(genes), int(out["bf_rounds"]), times[0], times[1])
    )


def synth(seed, L):
    lib = ctypes.CDLL(os.path.join(HERE, "_synth.so"))
    lib.phx_synth_contig.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_char_p]
    buf = ctypes.create_string_buffer(L)
    assert lib.phx_synth_contig(seed, L, buf) == 0
    return buf.raw.decode()


def save_fasta_gz(path, name, seq):
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write((">%s\n" % name).encode())
        for i in range(0, len(seq), 70):
            f.write((seq[i : i + 70] + "\n").encode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    os.system("gcc -O2 -shared -fPIC -o %s/_synth.so %s/phanotate_amd/csrc/phx_synth.c -lm" % (HERE, REPO))
    cases = []
    # the reference's own test inputs (data files, tests/*.fasta)
    for fn, nm in (("phiX174.fasta", "phiX174"), ("NC_001416.1.fasta", "NC_001416.1"), ("NC_000866.1.fasta", "NC_000866.1")):
        name, seq = read_fasta(os.path.join(REF, "tests", fn))
        cases.append((nm, name, seq, {}))
    for s in range(8):  # eight 50 kb contigs of the benchmark's generator: also the sample the reference's own speed is quoted on (ref_seconds)
        cases.append(("synth50k_%d" % s, "synth50k_%d" % s, synth(s, 50000), {}))
    for s in range(100, 104):
        cases.append(("synth6k_%d" % s, "synth6k_%d" % s, synth(s, 6000), {}))
    px = cases[0][2]
    rng = np.random.RandomState(7)
    cases.append(("edge_upper", "edge_upper", px.upper(), {}))
    cases.append(("edge_nrun", "edge_nrun", px[:1000] + "n" * 100 + px[1100:], {}))
    iu = list(px.lower())
    for p in rng.choice(len(iu), 60, replace=False):
        iu[p] = "ryswkmbvdh"[rng.randint(10)]
    cases.append(("edge_iupac", "edge_iupac", "".join(iu), {}))
    cases.append(("edge_badletter", "edge_badletter", px[:500] + "x" + px[501:], {}))
    cases.append(("edge_L5", "edge_L5", px[:5], {}))
    cases.append(("edge_L6", "edge_L6", px[:6], {}))
    cases.append(("edge_L80", "edge_L80", px[:80], {}))
    cases.append(("edge_L200", "edge_L200", px[:200], {}))
    cases.append(("edge_L1000", "edge_L1000", px[1000:2000], {}))
    lam = cases[1][2]
    cases.append(("edge_L4001", "edge_L4001", lam[20000:24001], {}))
    cases.append(("edge_L4002", "edge_L4002", lam[30001:34003], {}))
    # a long ORF-free stretch (>500 bp) forces the bridge edges of functions.py:320-354
    gapseq = "".join("tagctaactgattaa"[i % 15] for i in range(900))
    cases.append(("edge_bridge", "edge_bridge", lam[1000:4000] + gapseq + lam[4000:7000], {}))
    cases.append(("edge_bridge_left", "edge_bridge_left", gapseq + lam[4000:8000], {}))
    # an N run of 197 kb inside a contig: reading frames without a stop over 65 667 codons (the reference loops over any length,
    # functions.py:286-298; libphx keeps per-ORF class counts in 16 bits and counts such ORFs again in 32: VERDICT r2 #8)
    cases.append(("edge_longorf", "edge_longorf", synth(300, 8000) + "n" * 197000 + synth(301, 8000), {}))
    # path sums between 256 and 1088 bits: an open reading frame of 9000 sense codons (27 kb without a stop in frame 1,
    # ~130 in-frame start codons) between two ordinary stretches: |weight| ~ 1e150, beyond the CPU oracle's 256-bit integers, inside
    # the device's 512 / 1088-bit classes; the fixture's path comes from the generator's python-int Bellman-Ford over the reference's
    # own Decimal weights
    wr = np.random.RandomState(11)
    sense = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt" if a + b + c not in ("taa", "tag", "tga")]
    body = "".join(sense[i] for i in wr.randint(0, len(sense), 9000))
    cases.append(("edge_wide", "edge_wide", synth(310, 3000) + "atg" + body + "taa" + synth(311, 3000), {}))
    # path sums beyond the device's widest integers (missing #3): 21 000 sense codons without an in-frame start or stop
    # behind one atg (63 kb, one ORF of the frame): weight ~ 1e350 — more than a double holds, more than 1088 bits; the reference's
    # Decimal and the generator's python ints have no limit (CHANGELOG.md:11-13).  libphx solves such a contig on the host, in the
    # reference's own arithmetic (phx_exact.inc), instead of refusing it with PHX_S_OVERFLOW.
    wr = np.random.RandomState(12)
    quiet = [c for c in sense if c not in ("atg", "gtg", "ttg")]
    body2 = "".join(quiet[i] for i in wr.randint(0, len(quiet), 21000))
    cases.append(("edge_huge", "edge_huge", synth(320, 3000) + "atg" + body2 + "taa" + synth(321, 3000), {}))
    # non-default flags (file_handling.py:51-53)
    cases.append(("param_minlen60", "param_minlen60", synth(200, 6000), dict(minlen=60)))
    cases.append(("param_codons", "param_codons", synth(201, 6000), dict(start_codons="atg:0.7,gtg:0.2,ttg:0.05,ctg:0.05", stop_codons="tag,taa")))
    # the flag edges (file_handling.py:51-66, functions.py:186-215, 266): codons in two classes of the elif chain, atg not a start (only
    # the contig-end fragments that begin with atg train the GC frame plot), one stop, minlen around the multiples of 3 and beyond the
    # contig, 16 start codons, weights whose fp64 and Decimal quotients differ, the dict semantics of a repeated codon, zero and negative
    # weights.  The raw flag text is stored as flags_start / flags_stop (params_start is the reference's normalised dict).
    s21 = synth(421, 2400)
    # noatg: 100 sense codons behind the first base and in front of the last, on both strands, so that the fragments at the contig ends
    # (pseudo starts, functions.py:186-190, 241-242) are long ORFs whose first codon is atg: the only ORFs that train pos_max / pos_min
    wr = np.random.RandomState(13)
    rc = lambda x: x[::-1].translate(str.maketrans("acgt", "tgca"))
    orf_a = "atg" + "".join(sense[i] for i in wr.randint(0, len(sense), 100))
    orf_b = "atg" + "".join(sense[i] for i in wr.randint(0, len(sense), 100))
    pcases = [
        ("param_noatg", orf_a + synth(420, 2400) + rc(orf_b), dict(start_codons="gtg:1,ttg:0.5")),
        ("param_start_is_stop", s21, dict(start_codons="atg:1,tag:0.3")),
        ("param_start_rc_stop", synth(422, 3000), dict(start_codons="atg:1,cta:0.4,tta:0.2")),
        ("param_stop_rc_stop", synth(423, 2500), dict(stop_codons="tag,cta,taa")),
        ("param_one_stop", synth(424, 2000), dict(stop_codons="taa")),
        ("param_minlen6", synth(425, 1500), dict(minlen=6)),
        ("param_minlen7", synth(426, 1800), dict(minlen=7)),
        ("param_minlen91", synth(427, 3500), dict(minlen=91)),
        ("param_minlen92", synth(428, 3500), dict(minlen=92)),
        ("param_minlen_gt_contig", synth(429, 2000), dict(minlen=2500)),
        # (weights whose quotients by 0.8 end: libphx keeps a weight's text in 31 characters, and the suite hands it the normalised text)
        ("param_16_starts", synth(430, 4000), dict(start_codons="atg:0.8,gtg:0.1,ttg:0.05,ctg:0.04,att:0.02,ata:0.01,aca:0.008,gcc:0.004,"
                                                                  "cgc:0.002,tgt:0.001,ggg:0.0008,ccc:0.0004,aag:0.0002,gaa:0.0001,cag:0.4,agt:0.2")),
        ("param_weights_3_1", synth(431, 3000), dict(start_codons="atg:3,gtg:1,ttg:0.7")),
        ("param_repeated", synth(432, 3000), dict(start_codons="ATG:0.5,gtg:0.1,atg:1e-1,ttg:2E-2")),
        ("param_zero_weight", synth(433, 2500), dict(start_codons="atg:0.85,gtg:0,ttg:0.05")),
        ("param_negative_weight", synth(434, 2500), dict(start_codons="atg:0.85,gtg:-0.10,ttg:0.05")),
    ]
    for nm, seq, kw in pcases:
        cases.append((nm, nm, seq, kw))

    # tRNA masking (functions.py:457-509, connect branch 388-399) through a fake `aragorn` on PATH: (begin, end, complement)
    tr = {
        # both strands; the first within 2000 bp of the left end, the last of the right end (source / target edges)
        "trna_phiX174": ("phiX174", px, [(30, 104, False), (1200, 1275, False), (3000, 3080, True), (5290, 5370, True)]),
        # two hits 25 bp apart; hits whose ends fall on positions of ORF nodes of both strands; one inside a long gene
        "trna_lambda": ("NC_001416.1", lam, [(191, 265, False), (20000, 20075, False), (20100, 20180, False), (22686, 22760, True),
                                             (25396, 25470, True), (35000, 35090, False), (35070, 35150, True), (46400, 46475, True)]),
        "trna_synth6k": ("synth6k_100", synth(100, 6000), [(2500, 2572, True), (5800, 5890, False)]),
        # hits inside a 900 bp ORF-free stretch (the bridge case): nothing competes there, so tRNA edges end up ON the path
        "trna_gap": ("edge_bridge", lam[1000:4000] + gapseq + lam[4000:7000], [(3100, 3172, False), (3300, 3391, True), (3420, 3493, False), (3800, 3875, True)]),
        # the same hit twice: add_trnas adds the same edge again -> ValueError "parallel edges are forbidden" (graphs.py:74), the one
        # abort of the reference that an input can reach (libphx: per-contig status PHX_S_PARALLEL, the batch goes on)
        "trna_duplicate": ("synth6k_101", synth(101, 6000), [(2500, 2572, False), (4000, 4080, True), (2500, 2572, False)]),
        "trna_gap_left": ("edge_bridge_left", gapseq + lam[4000:8000], [(40, 112, True), (300, 372, False), (301, 380, False), (700, 771, False)]),
    }
    for nm, (name, seq, hits) in tr.items():
        cases.append((nm, name, seq, dict(trnas=hits)))

    for nm, name, seq, params in cases:
        if args.only and nm not in args.only:
            continue
        save_fasta_gz(os.path.join(HERE, nm + ".fasta.gz"), name, seq)
        make_case(nm, name, seq, HERE, **params)
    os.remove(os.path.join(HERE, "_synth.so"))


if __name__ == "__main__":
    main()
