#!/usr/bin/env python3
"""Cost of the re-annotation replacements (phx_rereplacements_flat) next to the run's own replacements (§13), same session.

    python tools/rereplace_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis), the run's replacements are computed (k_rp_*<.., DMarg>, the kernels as they were before the policy: the
          yardstick), then every contig is solved again with one called gene refused and one uncalled ORF penalised by 2.5 SCORE units
          (another pair every step), the margins of that re-annotation are computed, and then its replacements (its drop margins with the
          one-hop trees come with them: tools/redrops_time.py has their cost; then k_rp_*<.., MgDrop>).  Device times by the library's HIP
          events: argmin and walk of phx_rereplacements_ms next to those of phx_replacements_ms.  bound_ms = argmin + walk of
          phx_replacements_ms plus 15 %.
  lone    the same on the Lambda contig alone (tests/golden/NC_001416.1).

Exit status 1 when either measurement misses its bound."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(what, seqs, steps):
    import numpy as np

    import phanotate_amd as pa
    from phanotate_amd import _lib

    n = len(seqs)
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    st, offs, genes = ann.download_flat(exact=False)
    called, others = [], []
    oo = ann.orf_offsets()
    for i in range(n):
        cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3]
        c = [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[: steps + 1]] if st[i] == 0 else []
        called.append(c)
        n_orf = int(oo[i + 1] - oo[i])
        others.append([k for k in range(min(n_orf, 4 * steps + 8)) if k not in c][: steps + 1])  # (ORFs in orfs(i) order: the contig's left end)
    mask_of = lambda k: [[c[k % len(c)]] if c else None for c in called]
    bias_of = lambda k: [[(o[k % len(o)], 2.5)] if o else None for o in others]
    ann.replacements()  # warm-up: buffers allocated, kernels loaded
    ann.evidence(bias_of(steps), mask_of(steps), solve_all=True)
    ann.rereplacements()
    plain, cond, wall = [], [], []
    status = stats = out = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.replacements()
        plain.append(ann.replacements_ms())
        ann.evidence(bias_of(k), mask_of(k), solve_all=True)
        ann.remargins()
        t0 = time.perf_counter()
        out = ann.rereplacements()
        wall.append((time.perf_counter() - t0) * 1e3)
        status = out[0]
        cond.append(ann.rereplacements_ms())
        stats = (ann.replacement_stats(), ann.rereplacement_stats(), ann.redrop_stats())
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    p = {k: round(med([x[k] for x in plain]), 4) for k in plain[0]}
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    psum, csum = med([x["argmin"] + x["walk"] for x in plain]), med([x["argmin"] + x["walk"] for x in cond])
    V = int(bs["n_node"])
    R = stats[2]["slots"]  # (one record per pair of a path; the CDS genes are nearly all of them)
    ng = len(out[3])
    return {"what": what, "steps": steps, "rereplacements_device_ms": c, "replacements_device_ms": p, "rereplacements_sum_ms": round(csum, 4), "replacements_sum_ms": round(psum, 4),
            "rereplacements_wall_ms": round(med(wall), 4), "bound_ms": round(1.15 * psum, 4), "within_bound": bool(csum <= 1.15 * psum),
            "ratio": round(csum / psum, 4) if psum else None, "settled": int((status == 0).sum()), "replacement_stats": stats[0], "rereplacement_stats": stats[1],
            "nodes": V, "records": int(len(out[2])), "genes": ng,
            "extra_device_bytes": {"trees": 2 * 4 * (V + n + 1), "rounds": 4 * (V + n + 1), "chain": 4 * (V + 2), "per_record": (8 + 4 + 8 + 4 + 16 + 16 + _lib.REPL_DT.itemsize) * (R + 1),
                                   "genes": _lib.GENE_DT.itemsize * (ng + 1), "counters": 2 * 8 * 8}}


def main():
    import phanotate_amd as pa

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    batch = measure("batch: %d x %d bp, one called gene refused and one uncalled ORF penalised per contig, every contig solved again" % (a.n, a.len),
                    [pa.synth_contig(s, a.len) for s in range(a.n)], a.steps)
    print(json.dumps(batch), flush=True)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        lam = "".join(f.read().split("\n")[1:])
    lone = measure("lone: Lambda, one called gene refused and one uncalled ORF penalised", [lam], a.steps)
    print(json.dumps(lone), flush=True)
    return 0 if batch["within_bound"] and lone["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
