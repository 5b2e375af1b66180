#!/usr/bin/env python3
"""Cost of a pinned re-annotation (phx_constrain_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/constrain_time.py [--steps K]

One uncalled ORF per contig is required (an ORF some source -> target path runs through, by its margins record; another one every step,
so that no cached result is handed out) and every contig is solved again.  Per step: phx_run (wall), the constrain() call (wall), and the
library's HIP events around its device work (phx_reannotate_ms: mask build, solve, in-order parents + path + genes + copies).  In the same
session and on the same context: reannotate() with one called gene per contig refused — the masked solve, whose kernels the pinned
re-annotation leaves alone: the yardstick — and phx_run.  Medians of the steps; one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(steps, n, L):
    import numpy as np

    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, L) for s in range(n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    st, offs, genes = ann.download_flat(exact=False)
    mst, moffs, mrec = ann.margins()
    called, free = [], []
    for i in range(n):
        cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3]
        called.append([ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[: steps + 1]])
        rec = mrec[moffs[i]:moffs[i + 1]]
        pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1) & np.isfinite(rec["margin"]))[0]
        free.append(pool[:: max(1, len(pool) // (steps + 1))][: steps + 1].tolist())
    refuse = lambda k: [[c[k % len(c)]] if c else None for c in called]
    require = lambda k: [[c[k % len(c)]] if c else None for c in free]
    ann.reannotate(refuse(steps), solve_all=True)  # warm-up: buffers allocated, kernels loaded
    ann.constrain(None, require(steps), solve_all=True)
    med = lambda xs: float(np.median(xs))
    run_ms, c_wall, c_parts, r_wall, r_parts = [], [], [], [], []
    c_status, c_unmet, c_delta = None, None, None
    for k in range(steps):
        t0 = time.perf_counter()
        ann.run()
        run_ms.append((time.perf_counter() - t0) * 1e3)
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are neither call's cost)
        m = require(k)
        t0 = time.perf_counter()
        c_status, _, _, c_delta, c_unmet = ann.constrain(None, m, solve_all=True)
        c_wall.append((time.perf_counter() - t0) * 1e3)
        c_parts.append(ann.reannotate_ms())
        m = refuse(k)
        t0 = time.perf_counter()
        ann.reannotate(m, solve_all=True)
        r_wall.append((time.perf_counter() - t0) * 1e3)
        r_parts.append(ann.reannotate_ms())
    bs = ann.batch_sizes()
    nl = max(int(ann.globals(i).n_limbs) for i in range(n))
    ann.close()
    dev = lambda parts: {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    spread = lambda parts: round(float(np.max([p["solve"] for p in parts]) - np.min([p["solve"] for p in parts])), 4)
    cd, rd = dev(c_parts), dev(r_parts)
    return {"what": "pinned re-annotation of %d x %d bp, resident, one uncalled ORF per contig required, every contig solved again" % (n, L), "steps": steps,
            "phx_run_ms": round(med(run_ms), 4),
            "constrain_wall_ms": round(med(c_wall), 4), "constrain_device_ms": cd, "constrain_device_total_ms": round(sum(cd.values()), 4),
            "reannotate_wall_ms": round(med(r_wall), 4), "reannotate_device_ms": rd, "reannotate_device_total_ms": round(sum(rd.values()), 4),
            "solve_ratio": round(cd["solve"] / rd["solve"], 3) if rd["solve"] else None,
            "total_ratio": round(sum(cd.values()) / sum(rd.values()), 3) if sum(rd.values()) else None,
            "constrain_solve_spread_ms": spread(c_parts), "reannotate_solve_spread_ms": spread(r_parts),
            "negcycle": int((c_status == -9).sum()), "no_path": int((c_status == 1).sum()), "unmet": int(c_unmet.sum()),
            "delta_max": float(np.max(c_delta[np.isfinite(c_delta)])) if np.isfinite(c_delta).any() else None,
            "nodes": int(bs["n_node"]), "edges": int(bs["n_edge"]), "max_limbs": nl}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    print(json.dumps(measure(a.steps, a.n, a.len)), flush=True)


if __name__ == "__main__":
    main()
