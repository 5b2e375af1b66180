#!/usr/bin/env python3
"""Cost of the re-annotation profiles (phx_reprofile_flat) next to the run's own profiles (§34), same session.

    python tools/reprofile_time.py [--steps K] [--n N] [--len L]

Two measurements, one JSON line each (medians over the steps):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step the batch is run again (which drops
          every cached analysis), the run's profile is computed (k_pf_cand<NL>, k_pf_rec: the yardstick), then every contig is solved
          again with one called gene refused and one uncalled ORF penalised by 2.5 SCORE units (another pair every step: §21's setting),
          the margins of that re-annotation are computed (the conditioned d_t' is theirs, not this feature's cost), and then the profile
          of the re-annotation (k_pf_cand<NL, MgCond>, k_pf_rec<MgCond>).  Device times by the library's HIP events: tables / records /
          copy (phx_reprofile_ms) next to the same three of phx_profile_ms.  bound_ms = the run's tables figure plus 15 %.
  lone    the same on the Lambda contig alone (tests/golden/NC_001416.1).

Exit status 1 when the batch's conditioned tables figure misses its bound."""
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
    ann.profile()  # warm-up: buffers allocated, kernels loaded
    ann.evidence(bias_of(steps), mask_of(steps), solve_all=True)
    ann.remargins()
    ann.reprofile()
    plain, cond, wall = [], [], []
    status = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not this feature's cost)
        ann.profile()
        plain.append(ann.profile_ms())
        ann.evidence(bias_of(k), mask_of(k), solve_all=True)
        ann.remargins()  # (the conditioned reverse pass: §21's cost)
        t0 = time.perf_counter()
        status, poffs, prec = ann.reprofile()
        wall.append((time.perf_counter() - t0) * 1e3)
        cond.append(ann.reprofile_ms())
    slots = [int(poffs[i + 1] - poffs[i]) for i in range(n)]
    ann.close()
    med = lambda xs: float(np.median(xs))
    p = {k: round(med([x[k] for x in plain]), 4) for k in plain[0]}
    c = {k: round(med([x[k] for x in cond]), 4) for k in cond[0]}
    table = sum(cells(s) for s in slots if cells(s) > TAB_LDS) * 8
    return {"what": what, "steps": steps, "reprofile_device_ms": c, "profile_device_ms": p, "reprofile_wall_ms": round(med(wall), 4),
            "bound_ms": round(1.15 * p["tables"], 4), "within_bound": bool(c["tables"] <= 1.15 * p["tables"]),
            "tables_ratio": round(c["tables"] / p["tables"], 4) if p["tables"] else None,
            "settled": int((status == 0).sum()), "slots": int(sum(slots)), "contigs_in_global_memory": sum(1 for s in slots if cells(s) > TAB_LDS),
            "extra_device_bytes": {"tables": int(table), "records": 32 * (int(sum(slots)) + 1), "offsets": 8 * (2 * n + 2)}}


def main():
    import phanotate_amd as pa

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
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
