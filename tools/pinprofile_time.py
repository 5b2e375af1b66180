#!/usr/bin/env python3
"""Cost of the pinned profiles (phx_pinprofile_flat) next to the re-annotation profiles (§36), same session.

    python tools/pinprofile_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis) and the run's margins are computed (the out-edge CSR: shared, not this feature's cost).  Then
            yardstick  evidence() — one called gene refused, one uncalled ORF penalised by 2.5 SCORE units, every contig solved again —,
                       remargins() and reprofile(): k_pf_cand<NL, MgCond>, the parent's kernel (phx_reprofile_ms: tables);
            pinned     every contig solved again with one uncalled ORF some path runs through required (§24's setting), pinmargins()
                       (the pinned d_t' is theirs, not this feature's cost) and pinprofile(): k_pf_cand<NL, MgPinProf>
                       (phx_pinprofile_ms: tables), with the rounds it ran (phx_pinprofile_stats).
          allowance_ms = the yardstick x (rounds run / (3 x contigs covered)) x 3/2 x 1.15: each round is one pass over the edges, three
          limbs are moved and added where the yardstick has two, 15 % for the policy.
  lone    the same on the Lambda contig alone (tests/golden/NC_001416.1).

Exit status 1 when the batch's pinned tables figure misses its allowance."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAB_LDS = 4096  # PF_TAB_LDS


def cells(n):
    return n * n.bit_length()  # n (floor(log2 n) + 1)


def measure(what, seqs, steps):
    import numpy as np

    import phanotate_amd as pa

    n = len(seqs)
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    st, offs, genes = ann.download_flat(exact=False)
    mst, moffs, mrec = ann.margins()
    called, others = [], []
    for i in range(n):
        cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3]
        called.append([ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[: steps + 1]] if st[i] == 0 else [])
        rec = mrec[moffs[i]:moffs[i + 1]] if mst[i] == 0 else mrec[:0]
        others.append(np.nonzero((rec["called"] == 0) & (rec["through"] == 1))[0][: 2 * steps + 4].tolist())  # uncalled ORFs some path runs through
    mask_of = lambda k: [[c[k % len(c)]] if c else None for c in called]
    bias_of = lambda k: [[(o[(2 * k + 1) % len(o)], 2.5)] if o else None for o in others]
    req_of = lambda k: [[o[(2 * k) % len(o)]] if o else None for o in others]
    ann.evidence(bias_of(steps), mask_of(steps), solve_all=True)  # warm-up: buffers allocated, kernels loaded
    ann.remargins()
    ann.reprofile()
    ann.constrain(None, req_of(steps), solve_all=True)
    ann.pinmargins()
    ann.pinprofile()
    cond, pin, stats, wall = [], [], [], []
    status = lost = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.margins()
        ann.evidence(bias_of(k), mask_of(k), solve_all=True)
        ann.remargins()  # (the conditioned reverse pass: §21's cost)
        ann.reprofile()
        cond.append(ann.reprofile_ms())
        ann.constrain(None, req_of(k), solve_all=True)
        ann.pinmargins()  # (the pinned reverse pass: §24's cost)
        t0 = time.perf_counter()
        status, poffs, prec, lost = ann.pinprofile()
        wall.append((time.perf_counter() - t0) * 1e3)
        pin.append(ann.pinprofile_ms())
        stats.append(ann.pinprofile_stats())
    slots = [int(poffs[i + 1] - poffs[i]) for i in range(n)]
    ann.close()
    med = lambda xs: float(np.median(xs))
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    p = {k: round(med([x[k] for x in pin]), 4) for k in pin[0]}
    s = {k: int(med([x[k] for x in stats])) for k in stats[0]}
    ratio = s["rounds"] / (3.0 * s["contigs"]) if s["contigs"] else 1.0
    allowance = c["tables"] * ratio * 1.5 * 1.15
    table = sum(cells(x) for x in slots if cells(x) > TAB_LDS) * 8
    return {"what": what, "steps": steps, "pinprofile_device_ms": p, "reprofile_device_ms": c, "pinprofile_wall_ms": round(med(wall), 4), "stats": s,
            "yardstick_ms": c["tables"], "round_ratio": round(ratio, 4), "allowance_ms": round(allowance, 4), "pinned_tables_ms": p["tables"],
            "tables_ratio": round(p["tables"] / c["tables"], 4) if c["tables"] else None, "within_bound": bool(p["tables"] <= allowance),
            "settled": int((status == 0).sum()), "slots": int(sum(slots)), "slots_with_lost": int((lost > 0).any(axis=1).sum()),
            "contigs_in_global_memory": sum(1 for x in slots if cells(x) > TAB_LDS),
            "extra_device_bytes": {"tables": int(table), "records": 32 * (int(sum(slots)) + 1), "lost": 4 * (3 * int(sum(slots)) + 1), "rounds": 4 * (n + 1), "offsets": 8 * (2 * n + 2)}}


def main():
    import phanotate_amd as pa

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    batch = measure("batch: %d x %d bp, one uncalled ORF required per contig, every contig solved again" % (a.n, a.len), [pa.synth_contig(s, a.len) for s in range(a.n)], a.steps)
    print(json.dumps(batch), flush=True)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        lam = "".join(f.read().split("\n")[1:])
    print(json.dumps(measure("lone: Lambda, one uncalled ORF required", [lam], a.steps)), flush=True)
    return 0 if batch["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
