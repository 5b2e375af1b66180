#!/usr/bin/env python3
"""Cost of pinned scenario batches (phx_pinned_scenarios_flat).

    python tools/pinned_scenarios_time.py [--steps K] [--n N] [--len L] [--per-contig S] [--skip-lone] [--skip-batch]

Two measurements, medians over the steps, one JSON line each:

  lone    alt_starts() on the Lambda contig (tests/golden/NC_001416.1): one pinned scenario per (called gene, other start of its stop)
          in one call — device time (phx_scenarios_ms) and wall time — against the same questions asked one constrain() call each in a
          loop on the same context (summed phx_reannotate_ms and wall time).
  batch   N synthetic contigs of L bp resident, S pinned scenarios per contig (each requires one uncalled ORF some path runs through;
          another one every step, so that no cached result is handed out): solve ms per 1000 slot-solves against the pinned solve
          (k_rs_lds under the required policy) of constrain() on the same 1000 contigs in the same session — tools/constrain_time.py's figure, measured here on
          the same context as well — whose kernel this build leaves instruction for instruction as it was."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def lone(steps):
    import numpy as np

    import phanotate_amd as pa

    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        seq = "".join(f.read().split("\n")[1:])
    ann = pa.Annotator()
    ann.upload([seq])
    ann.run()
    st, offs, rec, soffs, genes = ann.alt_starts()  # warm-up: buffers, kernels, the drop margins
    alts = [int(k) for k in rec["alt"]]
    ann.constrain(None, [[alts[0]]])
    b_dev, b_wall, l_dev, l_wall, l_solve, b_solve = [], [], [], [], [], []
    for _ in range(steps):
        ann.run()
        ann.orf_offsets()
        ann.drop_margins()  # (alt_starts() builds on its records: not the scenarios' cost)
        t0 = time.perf_counter()
        st, offs, rec, soffs, genes = ann.alt_starts()
        t1 = time.perf_counter()
        ms = ann.scenarios_ms()
        b_wall.append((t1 - t0) * 1e3)
        b_dev.append(sum(ms.values()))
        b_solve.append(ms["solve"])
        dev = solve = 0.0
        deltas, stats, unmets = [], [], []
        t0 = time.perf_counter()
        for k in alts:
            cst, coffs, cgenes, delta, unmet = ann.constrain(None, [[k]])
            m = ann.reannotate_ms()
            dev += sum(m.values())
            solve += m["solve"]
            deltas.append(delta[0]); stats.append(cst[0]); unmets.append(unmet[0])
        l_wall.append((time.perf_counter() - t0) * 1e3)
        l_dev.append(dev)
        l_solve.append(solve)
        assert np.asarray(deltas).tobytes() == np.ascontiguousarray(rec["delta"]).tobytes()
        assert np.asarray(stats).tolist() == rec["status"].tolist() and np.asarray(unmets).tolist() == rec["unmet"].tolist()
    chunks = ann.scenario_chunks()
    ann.close()
    med = lambda xs: round(float(np.median(xs)), 4)
    return {"what": "alt_starts() on Lambda against one constrain() per (called gene, other start)", "steps": steps, "scenarios": len(alts), "genes": len(set(rec["orf"].tolist())),
            "chunks": chunks, "clean": int(((rec["status"] == 0) & (rec["unmet"] == 0)).sum()), "negcycle": int((rec["status"] == -9).sum()), "unmet": int((rec["unmet"] != 0).sum()),
            "batched_device_ms": med(b_dev), "batched_solve_ms": med(b_solve), "batched_wall_ms": med(b_wall),
            "loop_device_ms": med(l_dev), "loop_solve_ms": med(l_solve), "loop_wall_ms": med(l_wall),
            "device_ratio_loop_over_batched": round(med(l_dev) / max(med(b_dev), 1e-9), 2), "batched_below_loop": bool(med(b_dev) < med(l_dev))}


def batch(steps, n, L, per):
    import numpy as np

    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, L) for s in range(n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    mst, moffs, mrec = ann.margins()
    want = per + steps + 1
    free = []
    for i in range(n):
        rec = mrec[moffs[i]:moffs[i + 1]]
        pool = np.nonzero((rec["called"] == 0) & (rec["through"] == 1) & np.isfinite(rec["margin"]))[0]
        free.append(pool[:: max(1, len(pool) // want)][:want].tolist())
    scen_of = lambda k: [(i, None, [c[(k + s) % len(c)]]) for i, c in enumerate(free) if c for s in range(per)]
    req_of = lambda k: [[c[k % len(c)]] if c else None for c in free]
    ann.pinned_scenarios(scen_of(steps))  # warm-up
    ann.constrain(None, req_of(steps), solve_all=True)
    sc, sc_wall, rc, rc_wall = [], [], [], []
    slots = negcycle = 0
    for k in range(steps):
        ann.run()
        ann.orf_offsets()
        scen = scen_of(k)
        slots = len(scen)
        t0 = time.perf_counter()
        res = ann.pinned_scenarios(scen)
        sc_wall.append((time.perf_counter() - t0) * 1e3)
        sc.append(ann.scenarios_ms())
        negcycle = int((res[0] == -9).sum())
        m = req_of(k)
        t0 = time.perf_counter()
        ann.constrain(None, m, solve_all=True)
        rc_wall.append((time.perf_counter() - t0) * 1e3)
        rc.append(ann.reannotate_ms())
    chunks = ann.scenario_chunks()
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    sdev = {k: round(med([p[k] for p in sc]), 4) for k in sc[0]}
    rdev = {k: round(med([p[k] for p in rc]), 4) for k in rc[0]}
    per1000 = sdev["solve"] * 1000.0 / max(slots, 1)
    rper1000 = rdev["solve"] * 1000.0 / max(n, 1)
    return {"what": "%d x %d bp resident, %d pinned scenarios per contig, one uncalled ORF required each" % (n, L, per), "steps": steps, "slots": slots, "chunks": chunks,
            "negcycle_slots": negcycle, "scenarios_device_ms": sdev, "scenarios_wall_ms": round(med(sc_wall), 4), "solve_ms_per_1000_slots": round(per1000, 4),
            "constrain_device_ms": rdev, "constrain_wall_ms": round(med(rc_wall), 4), "constrain_solve_ms_per_1000_contigs": round(rper1000, 4),
            "bound_ms_per_1000": round(1.15 * rper1000, 4), "within_bound": bool(per1000 <= 1.15 * rper1000),
            "nodes": int(bs["n_node"]), "edges": int(bs["n_edge"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--per-contig", type=int, default=10)
    ap.add_argument("--skip-lone", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    a = ap.parse_args()
    if not a.skip_lone:
        print(json.dumps(lone(a.steps)), flush=True)
    if not a.skip_batch:
        print(json.dumps(batch(a.steps, a.n, a.len, a.per_contig)), flush=True)


if __name__ == "__main__":
    main()
