#!/usr/bin/env python3
"""Cost of scenario batches (phx_scenarios_flat).

    python tools/scenarios_time.py [--steps K] [--n N] [--len L] [--per-contig S] [--skip-lone] [--skip-batch]

Two measurements, medians over the steps, one JSON line each:

  lone    start_drops() on the Lambda contig (tests/golden/NC_001416.1): one scenario per called gene in one call — device time
          (phx_scenarios_ms) and wall time — against the same questions asked one reannotate() call each in a loop on the same context
          (summed phx_reannotate_ms and wall time).
  batch   N synthetic contigs of L bp resident, S scenarios per contig (each refuses one called gene; another gene every step, so that
          no cached result is handed out): solve ms per 1000 slot-solves against the masked solve (k_rs_lds) of reannotate() on the
          same 1000 contigs in the same session, whose kernel this build leaves instruction for instruction as it was."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def called_of(ann, i, st, offs, genes, limit=None):
    cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3]
    if limit is not None:
        cds = cds[:limit]
    return [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds]


def lone(steps):
    import numpy as np

    import phanotate_amd as pa

    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        seq = "".join(f.read().split("\n")[1:])
    ann = pa.Annotator()
    ann.upload([seq])
    ann.run()
    st, offs, rec, soffs, genes = ann.start_drops()  # warm-up: buffers, kernels, the drop margins
    orfs = [int(k) for k in rec["orf"]]
    ann.reannotate([[orfs[0]]])
    b_dev, b_wall, l_dev, l_wall, l_solve, b_solve = [], [], [], [], [], []
    for _ in range(steps):
        ann.run()
        ann.orf_offsets()
        ann.drop_margins()  # (start_drops() builds on its records: not the scenarios' cost)
        t0 = time.perf_counter()
        st, offs, rec, soffs, genes = ann.start_drops()
        t1 = time.perf_counter()
        ms = ann.scenarios_ms()
        b_wall.append((t1 - t0) * 1e3)
        b_dev.append(sum(ms.values()))
        b_solve.append(ms["solve"])
        dev = solve = 0.0
        drops = []
        t0 = time.perf_counter()
        for k in orfs:
            rst, roffs, rgenes, delta = ann.reannotate([[k]])
            m = ann.reannotate_ms()
            dev += sum(m.values())
            solve += m["solve"]
            drops.append(delta[0])
        l_wall.append((time.perf_counter() - t0) * 1e3)
        l_dev.append(dev)
        l_solve.append(solve)
        assert np.asarray(drops).tobytes() == np.ascontiguousarray(rec["drop"]).tobytes()
    chunks = ann.scenario_chunks()
    ann.close()
    med = lambda xs: round(float(np.median(xs)), 4)
    return {"what": "start_drops() on Lambda against one reannotate() per called gene", "steps": steps, "scenarios": len(orfs), "chunks": chunks,
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
    st, offs, genes = ann.download_flat(exact=False)
    called = [called_of(ann, i, st, offs, genes, per * 2 + steps + 1) for i in range(n)]
    scen_of = lambda k: [(i, [c[(k + s) % len(c)]]) for i, c in enumerate(called) if c for s in range(per)]
    mask_of = lambda k: [[c[k % len(c)]] if c else None for c in called]
    ann.scenarios(scen_of(steps))  # warm-up
    ann.reannotate(mask_of(steps), solve_all=True)
    sc, sc_wall, rs, rs_wall = [], [], [], []
    slots = 0
    for k in range(steps):
        ann.run()
        ann.orf_offsets()
        scen = scen_of(k)
        slots = len(scen)
        t0 = time.perf_counter()
        ann.scenarios(scen)
        sc_wall.append((time.perf_counter() - t0) * 1e3)
        sc.append(ann.scenarios_ms())
        m = mask_of(k)
        t0 = time.perf_counter()
        ann.reannotate(m, solve_all=True)
        rs_wall.append((time.perf_counter() - t0) * 1e3)
        rs.append(ann.reannotate_ms())
    chunks = ann.scenario_chunks()
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    sdev = {k: round(med([p[k] for p in sc]), 4) for k in sc[0]}
    rdev = {k: round(med([p[k] for p in rs]), 4) for k in rs[0]}
    per1000 = sdev["solve"] * 1000.0 / max(slots, 1)
    rper1000 = rdev["solve"] * 1000.0 / max(n, 1)
    return {"what": "%d x %d bp resident, %d scenarios per contig, one called gene refused each" % (n, L, per), "steps": steps, "slots": slots, "chunks": chunks,
            "scenarios_device_ms": sdev, "scenarios_wall_ms": round(med(sc_wall), 4), "solve_ms_per_1000_slots": round(per1000, 4),
            "reannotate_device_ms": rdev, "reannotate_wall_ms": round(med(rs_wall), 4), "reannotate_solve_ms_per_1000_contigs": round(rper1000, 4),
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
