#!/usr/bin/env python3
"""Cost of the pinned drop margins (phx_pindrops_flat) next to the re-annotation drop margins (§29), same session.

    python tools/pindrops_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis); every contig is solved again by evidence() with one uncalled ORF that some path runs through penalised
          by 2.5 SCORE units, its margins and then its drop margins are computed (k_dp_*<NL, MgDrop>, kernels this feature leaves as they
          were: the yardstick); then every contig is solved again by constrain() with that ORF required (another ORF every step), its
          pinned margins (the reverse pass on one limb more the drops build on: not this feature's cost) and then its pinned drop
          margins are computed (k_dp_*<NL, MgPinDrop>).  Device times by the library's HIP events: trees / candidates / fixups / copy of
          phx_pindrops_ms next to those of phx_redrops_ms.  bound_ms = the sum of the four parts of phx_redrops_ms x 3/2 (three limbs where
          there were two) x 1.15 (the policy), §24's allowance for the same change.
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
    ann.redrops()
    ann.constrain(None, pin_of(steps), solve_all=True)
    ann.pindrops()
    cond, pin, wall = [], [], []
    status = stats = unmet = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.evidence(bias_of(k), solve_all=True)
        ann.remargins()
        ann.redrops()
        cond.append(ann.redrops_ms())
        rstats = ann.redrop_stats()
        unmet = ann.constrain(None, pin_of(k), solve_all=True)[4]
        ann.pinmargins()
        t0 = time.perf_counter()
        status, _, rec, lost = ann.pindrops()
        wall.append((time.perf_counter() - t0) * 1e3)
        pin.append(ann.pindrops_ms())
        stats = (rstats, ann.pindrop_stats(), int((lost > 0).sum()), int(((lost > 0) & (rec["drop"] < 0)).sum()))
    ann.close()
    med = lambda xs: float(np.median(xs))
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    p = {k: round(med([x[k] for x in pin]), 4) for k in pin[0]}
    csum, psum = med([sum(x.values()) for x in cond]), med([sum(x.values()) for x in pin])
    worst = max(p, key=lambda k: p[k] - ALLOWANCE * c[k])
    return {"what": what, "steps": steps, "pindrops_device_ms": p, "redrops_device_ms": c, "pindrops_sum_ms": round(psum, 4), "redrops_sum_ms": round(csum, 4),
            "pindrops_wall_ms": round(med(wall), 4), "bound_ms": round(ALLOWANCE * csum, 4), "within_bound": bool(psum <= ALLOWANCE * csum),
            "ratio": round(psum / csum, 4) if csum else None, "part_ratios": {k: round(p[k] / c[k], 4) if c[k] else None for k in p}, "largest_excess": worst,
            "settled": int((status == 0).sum()), "unmet": int((unmet > 0).sum()), "redrop_stats": stats[0], "pindrop_stats": stats[1],
            "records_with_lost": stats[2], "of_them_negative": stats[3]}


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
