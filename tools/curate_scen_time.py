#!/usr/bin/env python3
"""Cost of combined scenario batches (phx_curate_scenarios_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/curate_scen_time.py [--steps K] [--n N] [--len L]

One slot per contig: one uncalled ORF required and another uncalled ORF with a bonus of 2.5 SCORE units (§22's choices: ORFs some
source -> target path runs through, by their margins records; other ones every step, so that no cached result is handed out) — every slot
is pinned AND biased and takes the table's fourth range.  In the same context and session the same slots go through pinned_scenarios()
without the bias: the pinned range, whose kernels this build leaves instruction for instruction as they were — the yardstick.  Per step
the library's HIP events around each call's device work (phx_scenarios_ms: slot records + marks, solve, in-order parents + path + genes +
copies) and the call's wall time.  Medians of the steps; one JSON line."""
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
    both = lambda k: [(i, [(c[(k + 1) % len(c)], -2.5)], None, [c[k % len(c)]]) for i, c in enumerate(free) if len(c) > 1]  # the next ORF of the list: never the required one
    pinned = lambda k: [(i, None, [c[k % len(c)]]) for i, c in enumerate(free) if len(c) > 1]
    ann.pinned_scenarios(pinned(steps))  # warm-up: buffers allocated, kernels loaded
    ann.curate_scenarios(both(steps))
    med = lambda xs: float(np.median(xs))
    c_wall, c_parts, p_wall, p_parts = [], [], [], []  # (c: curate_scenarios, p: pinned_scenarios)
    res, slots = None, 0
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are neither call's cost)
        scen = both(k)
        slots = len(scen)
        t0 = time.perf_counter()
        res = ann.curate_scenarios(scen)
        c_wall.append((time.perf_counter() - t0) * 1e3)
        c_parts.append(ann.scenarios_ms())
        chunks = ann.scenario_chunks()
        scen = pinned(k)
        t0 = time.perf_counter()
        ann.pinned_scenarios(scen)
        p_wall.append((time.perf_counter() - t0) * 1e3)
        p_parts.append(ann.scenarios_ms())
    bs = ann.batch_sizes()
    nl = max(int(ann.globals(i).n_limbs) for i in range(n))
    ann.close()
    dev = lambda parts: {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    spread = lambda parts: round(float(np.max([p["solve"] for p in parts]) - np.min([p["solve"] for p in parts])), 4)
    cd, pd = dev(c_parts), dev(p_parts)
    st, _, _, delta, unmet = res
    return {"what": "combined scenarios on %d x %d bp, resident, one slot per contig: one uncalled ORF required and one biased" % (n, L), "steps": steps, "slots": slots,
            "chunks": chunks, "curate_scenarios_wall_ms": round(med(c_wall), 4), "curate_scenarios_device_ms": cd, "curate_scenarios_device_total_ms": round(sum(cd.values()), 4),
            "pinned_scenarios_wall_ms": round(med(p_wall), 4), "pinned_scenarios_device_ms": pd, "pinned_scenarios_device_total_ms": round(sum(pd.values()), 4),
            "solve_ratio": round(cd["solve"] / pd["solve"], 3) if pd["solve"] else None, "solve_bound": 1.15, "within_bound": bool(pd["solve"] and cd["solve"] <= 1.15 * pd["solve"]),
            "total_ratio": round(sum(cd.values()) / sum(pd.values()), 3) if sum(pd.values()) else None,
            "curate_scenarios_solve_spread_ms": spread(c_parts), "pinned_scenarios_solve_spread_ms": spread(p_parts),
            "negcycle": int((st == -9).sum()), "no_path": int((st == 1).sum()), "unmet": int(unmet.sum()),
            "delta_max": float(np.max(delta[np.isfinite(delta)])) if np.isfinite(delta).any() else None,
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
