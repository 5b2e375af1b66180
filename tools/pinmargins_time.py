#!/usr/bin/env python3
"""Cost of the pinned margins (phx_pinmargins_flat) next to the re-annotation margins (§21), same session.

    python tools/pinmargins_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis) and the run's margins are computed (the out-edge CSR: shared, not this feature's cost).  Then
            yardstick  evidence() — one called gene refused, one uncalled ORF penalised by 2.5 SCORE units, every contig solved again —
                       and remargins(): k_sssp_rev<NL, MgCond>, the parent's kernel;
            constrain  every contig solved again with one uncalled ORF some path runs through required, and pinmargins():
                       k_pmg_apply, k_sssp_rev<NL, MgPin>, k_margins<NL, MgPin>;
            curate     the same with one further uncalled ORF penalised by 2.5 SCORE units.
          Device times by the library's HIP events: apply / reverse / records / copy (phx_pinmargins_ms, phx_remargins_ms).
          bound_ms = the yardstick's reverse pass x 3/2 (three limbs moved and added where it has two) x 1.15 (the policy).
  lone    the same on the Lambda contig alone (tests/golden/NC_001416.1).

Exit status 1 when a reverse pass of the batch misses its bound."""
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
    ann.curate(bias_of(steps), None, req_of(steps), solve_all=True)
    ann.pinmargins()
    cond, rows, wall = [], {"constrain": [], "curate": []}, {"constrain": [], "curate": []}
    status = {}
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.margins()
        ann.evidence(bias_of(k), mask_of(k), solve_all=True)
        ann.remargins()
        cond.append(ann.remargins_ms())
        for row in ("constrain", "curate"):
            if row == "constrain":
                ann.constrain(None, req_of(k), solve_all=True)
            else:
                ann.curate(bias_of(k), None, req_of(k), solve_all=True)
            t0 = time.perf_counter()
            status[row] = ann.pinmargins()[0]
            wall[row].append((time.perf_counter() - t0) * 1e3)
            rows[row].append(ann.pinmargins_ms())
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    bound = 1.5 * 1.15 * c["reverse"]
    out = {"what": what, "steps": steps, "remargins_device_ms": c, "bound_ms": round(bound, 4), "nodes": int(bs["n_node"]), "edges": int(bs["n_edge"])}
    ok = True
    for row in ("constrain", "curate"):
        p = {k: round(med([x[k] for x in rows[row]]), 4) for k in rows[row][0]}
        ok = ok and p["reverse"] <= bound
        out[row] = {"pinmargins_device_ms": p, "pinmargins_wall_ms": round(med(wall[row]), 4), "reverse_ratio": round(p["reverse"] / c["reverse"], 4) if c["reverse"] else None,
                    "within_bound": bool(p["reverse"] <= bound), "settled": int((status[row] == 0).sum())}
    out["within_bound"] = bool(ok)
    return out


def main():
    import phanotate_amd as pa

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    batch = measure("batch: %d x %d bp, one uncalled ORF required per contig (curate: and one penalised), every contig solved again" % (a.n, a.len),
                    [pa.synth_contig(s, a.len) for s in range(a.n)], a.steps)
    print(json.dumps(batch), flush=True)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        lam = "".join(f.read().split("\n")[1:])
    print(json.dumps(measure("lone: Lambda, one uncalled ORF required (curate: and one penalised)", [lam], a.steps)), flush=True)
    return 0 if batch["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
