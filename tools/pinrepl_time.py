#!/usr/bin/env python3
"""Cost of the pinned replacements (phx_pinreplacements_flat) next to the re-annotation replacements (§30), same session.

    python tools/pinrepl_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis); every contig is solved again by evidence() with one uncalled ORF that some path runs through penalised
          by 2.5 SCORE units, its margins, its drop margins and then its replacements are computed (k_rp_*<.., MgDrop>, kernels this
          feature leaves as they were: the yardstick); then every contig is solved again by constrain() with that ORF required (another
          ORF every step), its pinned margins and then its pinned replacements are computed (the pinned drop margins with the one-hop
          trees come with them: tools/pindrops_time.py has their cost; then k_rp_*<.., MgPinDrop>).  Device times by the library's HIP
          events: argmin and walk of phx_pinreplacements_ms next to those of phx_rereplacements_ms.  bound_ms = argmin + walk of
          phx_rereplacements_ms x 3/2 (three limbs where there were two) x 1.15 (the policy), §32's allowance for the same change.
          saturated: the records with lost > 0 — their slots' keys saturate in the 64-bit table, so a candidate that covers one walks its
          slot range before the exact compare; argmin_excess_ms = the pinned argmin minus 3/2 of the yardstick's bounds what those walks
          (and the policy's bitmap reads) cost.
  lone    the same on the Lambda contig alone (tests/golden/NC_001416.1).

Exit status 1 when the batch misses its bound."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALLOWANCE = 1.5 * 1.15


def measure(what, seqs, steps):
    import numpy as np

    import phanotate_amd as pa
    from phanotate_amd import _lib

    n = len(seqs)
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    mst, moffs, mrec = ann.margins()
    pool = []
    for i in range(n):
        rec = mrec[moffs[i]:moffs[i + 1]]
        ok = np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0] if mst[i] == 0 else []
        pool.append([int(k) for k in ok[:: max(1, len(ok) // (steps + 1))][: steps + 1]])  # (spread over the contig)
    pin_of = lambda k: [[p[k % len(p)]] if p else None for p in pool]
    bias_of = lambda k: [[(p[k % len(p)], 2.5)] if p else None for p in pool]
    ann.evidence(bias_of(steps), solve_all=True)  # warm-up: buffers allocated, kernels loaded
    ann.rereplacements()
    ann.constrain(None, pin_of(steps), solve_all=True)
    ann.pinreplacements()
    cond, pin, wall = [], [], []
    status = stats = unmet = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.evidence(bias_of(k), solve_all=True)
        ann.remargins()
        ann.rereplacements()
        cond.append(ann.rereplacements_ms())
        rstats = ann.rereplacement_stats()
        unmet = ann.constrain(None, pin_of(k), solve_all=True)[4]
        ann.pinmargins()
        t0 = time.perf_counter()
        status, _, rec, genes, lost = ann.pinreplacements()
        wall.append((time.perf_counter() - t0) * 1e3)
        pin.append(ann.pinreplacements_ms())
        stats = (rstats, ann.pinreplacement_stats(), int((lost > 0).sum()), int(((lost > 0) & (rec["drop"] < 0)).sum()), len(rec), len(genes), ann.pindrop_stats()["rescanned"])
    V = sum(int(ann.globals(i).n_node) for i in range(n))
    ann.close()
    med = lambda xs: float(np.median(xs))
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    p = {k: round(med([x[k] for x in pin]), 4) for k in pin[0]}
    part = lambda x: x["argmin"] + x["walk"]
    csum, psum = med([part(x) for x in cond]), med([part(x) for x in pin])
    nv = V + n + 1
    mem = {"trees": 2 * 4 * nv, "settle_rounds": 4 * nv, "chain": 4 * (V + 2), "per_record_112": 112 * (stats[4] + 1), "genes": _lib.GENE_DT.itemsize * (stats[5] + 1)}
    return {"what": what, "steps": steps, "pinreplacements_device_ms": p, "rereplacements_device_ms": c, "pinreplacements_sum_ms": round(psum, 4), "rereplacements_sum_ms": round(csum, 4),
            "pinreplacements_wall_ms": round(med(wall), 4), "bound_ms": round(ALLOWANCE * csum, 4), "within_bound": bool(psum <= ALLOWANCE * csum),
            "ratio": round(psum / csum, 4) if csum else None, "part_ratios": {k: round(p[k] / c[k], 4) if c[k] else None for k in p},
            "argmin_excess_ms": round(p["argmin"] - 1.5 * c["argmin"], 4), "settled": int((status == 0).sum()), "unmet": int((unmet > 0).sum()),
            "rereplacement_stats": stats[0], "pinreplacement_stats": stats[1], "records": stats[4], "genes": stats[5], "saturated": stats[2], "of_them_negative": stats[3],
            "rescanned": stats[6], "nodes": V, "device_bytes": mem, "device_mb": round(sum(mem.values()) / 1e6, 1)}


def main():
    import phanotate_amd as pa

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    batch = measure("batch: %d x %d bp, one uncalled ORF that some path runs through required per contig, every contig solved again" % (a.n, a.len),
                    [pa.synth_contig(s, a.len) for s in range(a.n)], a.steps)
    print(json.dumps(batch), flush=True)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        lam = "".join(f.read().split("\n")[1:])
    lone = measure("lone: Lambda, one uncalled ORF that some path runs through required", [lam], a.steps)
    print(json.dumps(lone), flush=True)
    return 0 if batch["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
