#!/usr/bin/env python3
"""Cost of the per-ORF path margins (phx_margins_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/margins_time.py [--steps K] [--trace OUTDIR]

Per step: phx_run (wall), then the first margins call after it (wall), split by the library's HIP events into the out-edge CSR
(k_mg_count / k_mg_scan / k_mg_fill), the reverse pass (k_sssp_rev), the records (k_margins) and their copy to the host; the rest of
the wall time is the host (permutation to iter_orfs order, `called`).  Prints one JSON line, with the extra device memory of the pass.
--trace OUTDIR: afterwards, in a separate child process, `rocprofv3 --kernel-trace --stats` over a few steps, and the stats rows of the
new kernels."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = ("k_mg_count", "k_mg_scan", "k_mg_fill", "k_sssp_rev", "k_margins")


def measure(steps, n, L):
    import numpy as np

    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, L) for s in range(n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    ann.download_flat()
    ann.margins()  # warm-up: buffers of the pass allocated, kernels loaded
    run_ms, wall_ms, parts = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ann.run()
        t1 = time.perf_counter()
        ann.download_flat()  # (the certificate and the delivered genes the margins compare against: not part of the margins' cost)
        t2 = time.perf_counter()
        st, offs, rec = ann.margins()
        t3 = time.perf_counter()
        run_ms.append((t1 - t0) * 1e3)
        wall_ms.append((t3 - t2) * 1e3)
        parts.append(ann.margins_ms())
    bs = ann.batch_sizes()
    n_orf, n_node, n_edge = bs["n_orf"], bs["n_node"], bs["n_edge"]
    nl = max(int(ann.globals(i).n_limbs) for i in range(n))
    extra = (n_node + n + 1) * 4 + n_edge * 12 + n_node * nl * 8 + n_orf * 40 + n * 4
    med = lambda xs: float(np.median(xs))
    dev = {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    out = {"what": "margins call on %d x %d bp, resident" % (n, L), "steps": steps, "phx_run_ms": round(med(run_ms), 4), "margins_wall_ms": round(med(wall_ms), 4),
           "margins_device_ms": dev, "margins_device_total_ms": round(sum(dev.values()), 4), "host_ms": round(med(wall_ms) - sum(dev.values()), 4),
           "orfs": int(n_orf), "through": int(rec["through"].sum()), "nodes": int(n_node), "edges": int(n_edge), "max_limbs": nl, "extra_device_bytes": int(extra)}
    ann.close()
    return out


def trace(outdir, steps, n, L):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "margins", "--", sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--n", str(n), "--len", str(L)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr[-4000:])
        return {"trace_rc": r.returncode}
    rows = {}
    for fn in glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True):
        with open(fn) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if any(k in name for k in KERNELS):
                    rows[name.split("(")[0]] = {c: row[c] for c in ("Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs") if c in row}
    return {"kernel_stats": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    ap.add_argument("--trace", default=None, help="directory for a separate rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    print(json.dumps(measure(a.steps, a.n, a.len)), flush=True)
    if a.trace:
        print(json.dumps(trace(a.trace, 3, a.n, a.len)), flush=True)


if __name__ == "__main__":
    main()
