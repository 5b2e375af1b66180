#!/usr/bin/env python3
"""Cost of a combined re-annotation (phx_curate_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/curate_time.py [--steps K]

One uncalled ORF per contig is required and another uncalled ORF gets a bonus (ORFs some source -> target path runs through, by their
margins records; other ones every step, so that no cached result is handed out) and every contig is solved again.  Per step: phx_run
(wall), the curate() call (wall), and the library's HIP events around its device work (phx_reannotate_ms: mask build, solve, in-order
parents + path + genes + copies).  In the same session and on the same context: constrain() with the same required ORF and no bias — the
pinned solve, whose kernels the combined re-annotation leaves alone: the yardstick (tools/constrain_time.py measures it on its own) — and
phx_run.  Medians of the steps; one JSON line."""
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
    ann.download_flat(exact=False)
    mst, moffs, mrec = ann.margins()
    free = []
    for i in range(n):
        rec = mrec[moffs[i]:moffs[i + 1]]
        pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1) & np.isfinite(rec["margin"]))[0]
        free.append(pool[:: max(1, len(pool) // (steps + 1))][: steps + 1].tolist())
    require = lambda k: [[c[k % len(c)]] if c else None for c in free]
    bonus = lambda k: [[(c[(k + 1) % len(c)], -2.5)] if len(c) > 1 else None for c in free]  # the next ORF of the list: never the required one
    ann.constrain(None, require(steps), solve_all=True)  # warm-up: buffers allocated, kernels loaded
    ann.curate(bonus(steps), None, require(steps), solve_all=True)
    med = lambda xs: float(np.median(xs))
    run_ms, c_wall, c_parts, r_wall, r_parts = [], [], [], [], []  # (c: curate, r: constrain)
    c_status, c_unmet, c_delta = None, None, None
    for k in range(steps):
        t0 = time.perf_counter()
        ann.run()
        run_ms.append((time.perf_counter() - t0) * 1e3)
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are neither call's cost)
        m, b = require(k), bonus(k)
        t0 = time.perf_counter()
        c_status, _, _, c_delta, c_unmet = ann.curate(b, None, m, solve_all=True)
        c_wall.append((time.perf_counter() - t0) * 1e3)
        c_parts.append(ann.reannotate_ms())
        t0 = time.perf_counter()
        ann.constrain(None, m, solve_all=True)
        r_wall.append((time.perf_counter() - t0) * 1e3)
        r_parts.append(ann.reannotate_ms())
    bs = ann.batch_sizes()
    nl = max(int(ann.globals(i).n_limbs) for i in range(n))
    ann.close()
    dev = lambda parts: {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    spread = lambda parts: round(float(np.max([p["solve"] for p in parts]) - np.min([p["solve"] for p in parts])), 4)
    cd, rd = dev(c_parts), dev(r_parts)
    return {"what": "combined re-annotation of %d x %d bp, resident, one uncalled ORF per contig required and one biased, every contig solved again" % (n, L), "steps": steps,
            "phx_run_ms": round(med(run_ms), 4),
            "curate_wall_ms": round(med(c_wall), 4), "curate_device_ms": cd, "curate_device_total_ms": round(sum(cd.values()), 4),
            "constrain_wall_ms": round(med(r_wall), 4), "constrain_device_ms": rd, "constrain_device_total_ms": round(sum(rd.values()), 4),
            "solve_ratio": round(cd["solve"] / rd["solve"], 3) if rd["solve"] else None, "solve_bound": 1.15,
            "total_ratio": round(sum(cd.values()) / sum(rd.values()), 3) if sum(rd.values()) else None,
            "curate_solve_spread_ms": spread(c_parts), "constrain_solve_spread_ms": spread(r_parts),
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
