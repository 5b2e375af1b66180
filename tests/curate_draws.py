"""Shared by tests/test_curate_host.py and tests/test_curate_gpu.py: the contigs of the random mixes, their graphs as the CPU
oracle builds them, and the seeded draws of required, biased and refused ORFs.  An ORF is named by (left, right, strand) as a gene row
prints it, which is the same on the oracle's graph and on the device's, so the host test can count on the CPU how many draws settle and
the GPU test can hand the very same draws to the device."""
import os
import sys

import numpy as np

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUNDS = 5  # x 9 contigs = 45 draws
SEED = 2201


def mix_seqs(pa):
    """test_scenarios_gpu.case1_seqs + fuzz(11, 6), as bytes or str as the annotator takes them."""
    import fuzz_gpu

    rng = np.random.RandomState(11)
    return [pa.synth_contig(71, 20000), pa.synth_contig(72, 9000), load_golden("phiX174")[2]] + [fuzz_gpu.make(rng) for _ in range(6)]


class OracleGraph:
    """One contig's graph from the CPU oracle: edges [(u, v, W)] in the oracle's edge order, W the exact integer trunc(w * 1000); the ORF
    edges by (left, right, strand); the keys of the genes the oracle's own path calls.  None-like (ok False) where the oracle has no path.
    `params` (oracle.make_params) and `trnas` (the hit list) go to oracle.run as they are; a tRNA node (frame +-4) is never an ORF's."""

    def __init__(self, orc, seq, params=None, trnas=None):
        r = orc.run(seq, params, trnas=trnas)
        self.ok = r["status"] == 0 and "path" in r and len(r["path"]) >= 2 and not r["wide"]
        if not self.ok:
            return
        typ, frame, pos = r["node_type"].tolist(), r["node_frame"].tolist(), r["node_pos"].tolist()
        self.V, self.type, self.frame = len(typ), typ, frame
        self.src, self.tgt = typ.index(2), typ.index(3)
        w = [orc.limbs_to_int(x) for x in r["edge_wint_limbs"]]
        self.edges = list(zip(r["edge_src"].tolist(), r["edge_dst"].tolist(), w))
        self.orf_edge = {}
        for u, v, _ in self.edges:
            if typ[u] > 1 or typ[v] > 1 or abs(frame[u]) > 3 or frame[u] != frame[v]:
                continue
            # an ORF edge runs start -> stop on the forward strand and stop -> start on the reverse one (a connector the other way round)
            if (frame[u] > 0 and typ[u] == 0 and typ[v] == 1) or (frame[u] < 0 and typ[u] == 1 and typ[v] == 0):
                self.orf_edge[(pos[u], pos[v] + 2, 1 if frame[u] > 0 else -1)] = (u, v)
        self.called = {(int(a), int(b), int(s)) for a, b, s, f in zip(r["gene_left"], r["gene_right"], r["gene_strand"], r["gene_frame"]) if abs(int(f)) <= 3}
        self.D = r["path_dist"]


def draw(keys, called, rng):
    """One mix over a contig whose ORF edges are `keys` (sorted) and whose called ORFs are `called`: 1-2 required uncalled ORFs, 1-3 biased
    ORFs of both signs (|B| from a hundredth of a SCORE unit to thirty units; a called gene among them now and then, and sometimes a required
    ORF itself), 0-2 refused ORFs (called genes mostly), never one that is required."""
    uncalled = [k for k in keys if k not in called]
    cg = [k for k in keys if k in called]
    pick = lambda pool, m: [pool[j] for j in sorted(rng.choice(len(pool), min(m, len(pool)), replace=False).tolist())]
    require = pick(uncalled, int(rng.randint(1, 3)))
    nb = int(rng.randint(1, 4))
    pool = (cg if cg and rng.rand() < 0.4 else keys)
    biased = pick(pool, nb)
    if rng.rand() < 0.3:
        biased[0] = require[0]
    bias = {}
    for j, k in enumerate(biased):
        sign = -1 if j == 0 else (1 if j == 1 else int(rng.choice([-1, 1])))  # both signs whenever there are two
        bias[k] = sign * int(10 ** rng.uniform(1.0, 4.5))
    nf = int(rng.randint(0, 3))
    pool = [k for k in (cg if cg and rng.rand() < 0.7 else keys) if k not in require]
    forbid = pick(pool, nf) if pool else []
    return dict(require=require, bias=bias, forbid=forbid)


def mixes(graphs):
    """ROUNDS draws per usable contig: [round][contig] -> draw() or None.  `graphs`: per contig an object with .ok, .orf_edge (a dict by
    key) and .called."""
    rng = np.random.RandomState(SEED)
    out = []
    for _ in range(ROUNDS):
        row = []
        for g in graphs:
            keys = sorted(g.orf_edge) if g.ok else []
            row.append(draw(keys, g.called, rng) if len(keys) >= 4 and any(k not in g.called for k in keys) else None)
        out.append(row)
    return out


def weights(edges, orf_edge, d, M):
    """The edge list of a draw: refused rows taken out, W + B on the biased ones, - M on the required ones (the set R')."""
    gone = {orf_edge[k] for k in d["forbid"] if k in orf_edge}
    pinned = {orf_edge[k] for k in d["require"] if k in orf_edge} - gone
    add = {}
    for k, B in d["bias"].items():
        if k in orf_edge:
            add[orf_edge[k]] = add.get(orf_edge[k], 0) + B
    return [(u, v, w + add.get((u, v), 0) - (M if (u, v) in pinned else 0)) for u, v, w in edges if (u, v) not in gone], pinned


def big_m(edges, d):
    """Above every walk sum: 1 + sum |W| + sum |B|."""
    return 1 + sum(abs(w) for _, _, w in edges) + sum(abs(B) for B in d["bias"].values())
