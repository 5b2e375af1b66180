#!/usr/bin/env python3
"""Cost of the re-annotation margins (phx_remargins_flat) next to the run's own margins (§11), same session.

    python tools/remargins_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis), the run's margins are computed (k_mg_*, k_sssp_rev<NL>, k_margins<NL>: the yardstick), then every contig
          is solved again with one called gene refused and one uncalled ORF penalised by 2.5 SCORE units (another pair every step), and the
          margins of that re-annotation are computed (k_rmg_apply, k_sssp_rev<NL, MgCond>, k_margins<NL, MgCond>).  Device times by the
          library's HIP events: apply / reverse / records / copy (phx_remargins_ms) next to transpose / reverse / records / copy
          (phx_margins_ms), and k_rs_mask's time on the same inputs, under the bias mode, (phx_reannotate_ms) next to k_rmg_apply's.
          bound_ms = the unconditioned reverse pass plus 15 %.
  lone    the same on the Lambda contig alone (tests/golden/NC_001416.1).

Exit status 1 when the batch's conditioned reverse pass misses its bound."""
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
    ann.margins()  # warm-up: buffers allocated, kernels loaded
    ann.evidence(bias_of(steps), mask_of(steps), solve_all=True)
    ann.remargins()
    plain, cond, ev, wall = [], [], [], []
    status = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.margins()
        plain.append(ann.margins_ms())
        ann.evidence(bias_of(k), mask_of(k), solve_all=True)
        ev.append(ann.reannotate_ms())
        t0 = time.perf_counter()
        status = ann.remargins()[0]
        wall.append((time.perf_counter() - t0) * 1e3)
        cond.append(ann.remargins_ms())
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    p = {k: round(med([x[k] for x in plain]), 4) for k in plain[0]}
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    V, E, N = int(bs["n_node"]), int(bs["n_edge"]), int(bs["n_orf"])
    limbs = 2  # (both inputs are 128-bit batches; a wider batch keeps its widest class's limbs per node)
    return {"what": what, "steps": steps, "remargins_device_ms": c, "margins_device_ms": p, "remargins_wall_ms": round(med(wall), 4),
            "bound_ms": round(1.15 * p["reverse"], 4), "within_bound": bool(c["reverse"] <= 1.15 * p["reverse"]),
            "reverse_ratio": round(c["reverse"] / p["reverse"], 4) if p["reverse"] else None,
            "apply_ms": c["apply"], "k_rs_mask_ms": round(med([x["mask"] for x in ev]), 4),
            "settled": int((status == 0).sum()), "nodes": V, "edges": E,
            "extra_device_bytes": {"bitmaps": 2 * (E // 32 + 2) * 4, "bias_words": 8 * (E + 1), "dist_t": 8 * limbs * (V + 1), "records": 40 * (N + 1), "per_contig": 8 * (n + 1)}}


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
    print(json.dumps(measure("lone: Lambda, one called gene refused and one uncalled ORF penalised", [lam], a.steps)), flush=True)
    return 0 if batch["within_bound"] else 1


if __name__ == "__main__":
    sys.exit(main())
