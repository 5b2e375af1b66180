#!/usr/bin/env python3
"""Cost of evidence scenario batches (phx_evidence_scenarios_flat).

    python tools/evidence_scenarios_time.py [--steps K] [--n N] [--len L] [--per-contig S] [--skip-lone] [--skip-batch]

Two measurements, medians over the steps, one JSON line each:

  lone    evidence_scan() on the Lambda contig (tests/golden/NC_001416.1): per called gene one ORF of its stop group (another start where
          the group has one, else the gene's own) with a bonus of 5 SCORE units, every hit a scenario of one call — device time
          (phx_scenarios_ms) and wall time — against the same questions asked one evidence() call each in a loop on the same context
          (summed phx_reannotate_ms and wall time).  The deltas must be equal.  Beside it one scenario with a penalty on every ORF of
          Lambda: the longest list the contig can give, sorted by counting in one workgroup (full_list_device_ms, "mask" holds the sort).
  batch   N synthetic contigs of L bp resident, S scenarios per contig (each puts a bonus of 2.5 SCORE units on one uncalled ORF; another
          ORF every step, so that no cached result is handed out): solve ms per 1000 slot-solves against the biased solve (k_rs_lds under the bias policy) of
          evidence() on the same contigs in the same session (one ORF per contig biased, as tools/evidence_time.py measures it), and the
          bytes of a biased slot against a dense slice of one word per in-edge slot.

The two bounds are requirements: the tool exits non-zero when the batched device time is not below the loop's or the batch figure is
beyond the sibling's plus 15 %."""
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
    st, offs, genes = ann.download_flat(exact=False)
    group = ann.orfs(0)["group"]
    hits = []
    for g in genes:
        if abs(int(g["frame"])) > 3:
            continue
        k = ann.orf_index(0, int(g["left"]), int(g["right"]), int(g["strand"]))
        alts = [int(a) for a in np.nonzero(group == group[k])[0] if a != k]
        hits.append((alts[0] if alts else k, -5.0))
    ann.evidence_scan([hits])  # warm-up: buffers, kernels
    ann.evidence([[hits[0]]], solve_all=True)
    b_dev, b_wall, b_solve, l_dev, l_wall, l_solve = [], [], [], [], [], []
    moved = cycles = 0
    for _ in range(steps):
        ann.run()
        ann.orf_offsets()
        t0 = time.perf_counter()
        st, offs, rec, soffs, sgenes = ann.evidence_scan([hits])
        t1 = time.perf_counter()
        ms = ann.scenarios_ms()
        b_wall.append((t1 - t0) * 1e3)
        b_dev.append(sum(ms.values()))
        b_solve.append(ms["solve"])
        dev = solve = 0.0
        deltas = []
        t0 = time.perf_counter()
        for h in hits:
            est, eoffs, egenes, delta = ann.evidence([[h]], solve_all=True)
            m = ann.reannotate_ms()
            dev += sum(m.values())
            solve += m["solve"]
            deltas.append(delta[0])
        l_wall.append((time.perf_counter() - t0) * 1e3)
        l_dev.append(dev)
        l_solve.append(solve)
        assert np.asarray(deltas).tobytes() == np.ascontiguousarray(rec["delta"]).tobytes()
        moved, cycles = int((rec["delta"] < 0).sum()), int((rec["status"] == -9).sum())
    chunks = ann.scenario_chunks()
    # the longest list a contig can give: a small penalty on every ORF in one scenario (k_sce_sort ranks it by counting)
    n_orf = int(ann.orf_offsets()[1])
    full = []
    for _ in range(steps):
        ann.run()
        ann.orf_offsets()
        ann.evidence_scenarios([(0, [(k, 0.003) for k in range(n_orf)], None)])
        full.append(ann.scenarios_ms())
    ann.close()
    med = lambda xs: round(float(np.median(xs)), 4)
    full_ms = {k: med([p[k] for p in full]) for k in full[0]}
    return {"full_list_orfs": n_orf, "full_list_device_ms": full_ms, "what": "evidence_scan() on Lambda, one hit per called gene's stop group, against one evidence() per hit", "steps": steps, "scenarios": len(hits), "chunks": chunks,
            "moved": moved, "negcycle": cycles, "batched_device_ms": med(b_dev), "batched_solve_ms": med(b_solve), "batched_wall_ms": med(b_wall),
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
    oo = ann.orf_offsets()
    others = []
    for i in range(n):
        cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3] if st[i] == 0 else []
        c = {ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[: 4 * (per + steps) + 8]}
        n_orf = int(oo[i + 1] - oo[i])
        others.append([k for k in range(min(n_orf, 4 * (per + steps) + 8)) if k not in c][: per + steps + 1])  # (ORFs in orfs(i) order: the contig's left end)
    scen_of = lambda k: [(i, [(o[(k + s) % len(o)], -2.5)], None) for i, o in enumerate(others) if o for s in range(per)]
    bias_of = lambda k: [[(o[k % len(o)], -2.5)] if o else None for o in others]
    ann.evidence_scenarios(scen_of(steps))  # warm-up
    ann.evidence(bias_of(steps), solve_all=True)
    sc, sc_wall, ev, ev_wall = [], [], [], []
    slots = 0
    for k in range(steps):
        ann.run()
        ann.orf_offsets()
        scen = scen_of(k)
        slots = len(scen)
        t0 = time.perf_counter()
        ann.evidence_scenarios(scen)
        sc_wall.append((time.perf_counter() - t0) * 1e3)
        sc.append(ann.scenarios_ms())
        b = bias_of(k)
        t0 = time.perf_counter()
        ann.evidence(b, solve_all=True)
        ev_wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(ann.reannotate_ms())
    chunks = ann.scenario_chunks()
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    sdev = {k: round(med([p[k] for p in sc]), 4) for k in sc[0]}
    edev = {k: round(med([p[k] for p in ev]), 4) for k in ev[0]}
    per1000 = sdev["solve"] * 1000.0 / max(slots, 1)
    eper1000 = edev["solve"] * 1000.0 / max(n, 1)
    E = int(bs["n_edge"]) // max(n, 1)
    return {"what": "%d x %d bp resident, %d scenarios per contig, one uncalled ORF with a bonus each" % (n, L, per), "steps": steps, "slots": slots, "chunks": chunks,
            "scenarios_device_ms": sdev, "scenarios_wall_ms": round(med(sc_wall), 4), "solve_ms_per_1000_slots": round(per1000, 4),
            "evidence_device_ms": edev, "evidence_wall_ms": round(med(ev_wall), 4), "evidence_solve_ms_per_1000_contigs": round(eper1000, 4),
            "bound_ms_per_1000": round(1.15 * eper1000, 4), "within_bound": bool(per1000 <= 1.15 * eper1000),
            "nodes": int(bs["n_node"]), "edges": int(bs["n_edge"]),
            "biased_slot_extra_bytes": (E // 32 + 3) * 4 + 40 + 48, "dense_slice_bytes": 8 * E}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--per-contig", type=int, default=10)
    ap.add_argument("--skip-lone", action="store_true")
    ap.add_argument("--skip-batch", action="store_true")
    a = ap.parse_args()
    missed = []
    if not a.skip_lone:
        r = lone(a.steps)
        print(json.dumps(r), flush=True)
        if not r["batched_below_loop"]:
            missed.append("lone: the batched device time is not below the loop's")
    if not a.skip_batch:
        r = batch(a.steps, a.n, a.len, a.per_contig)
        print(json.dumps(r), flush=True)
        if not r["within_bound"]:
            missed.append("batch: the solve per 1000 slots is beyond the biased k_rs_lds' per 1000 contigs plus 15 %")
    if missed:  # the two bounds are requirements (Cost)
        sys.exit("; ".join(missed))


if __name__ == "__main__":
    main()
