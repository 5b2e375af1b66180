#!/usr/bin/env python3
"""Cost of the gene drop margins (phx_drop_margins_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/drop_time.py [--steps K] [--trace OUTDIR]

Per step: phx_run (wall), then the shared part of the margins (out-edge CSR and reverse pass, through phx_tap_dist_target: wall, and
its device time from phx_margins_ms), then the first drop-margins call after it (wall), split by the library's HIP events into trees + labels (k_dp_tree),
candidates + sparse table (k_dp_cand), fixups (k_dp_rescan, k_dp_cross, k_dp_rec) and the copy of the records; the rest of the wall time
is the host (`called`, compaction, the Python array).  Prints one JSON line with phx_drop_stats and the extra device memory.
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

KERNELS = ("k_mg_count", "k_mg_scan", "k_mg_fill", "k_sssp_rev", "k_dp_tree", "k_dp_cand", "k_dp_rescan", "k_dp_cross", "k_dp_rec")


def measure(steps, n, L):
    import ctypes as C

    import numpy as np

    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, L) for s in range(n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    ann.download_flat()
    ann.drop_margins()  # warm-up: buffers of the pass allocated, kernels loaded
    g0 = ann.globals(0)
    dt0 = np.zeros((max(int(g0.n_node), 1), max(int(g0.n_limbs), 1)), np.uint64)
    run_ms, rev_ms, wall_ms, parts, rev_parts = [], [], [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ann.run()
        t1 = time.perf_counter()
        ann.download_flat()  # (the certificate and the delivered genes `called` compares against: not part of the drops' cost)
        t2 = time.perf_counter()
        ann.L.phx_tap_dist_target(ann.h, 0, dt0.ctypes.data_as(C.c_void_p), dt0.size)  # the shared part alone: out-edge CSR, reverse pass
        t3 = time.perf_counter()
        st, offs, rec = ann.drop_margins()
        t4 = time.perf_counter()
        run_ms.append((t1 - t0) * 1e3)
        rev_ms.append((t3 - t2) * 1e3)
        wall_ms.append((t4 - t3) * 1e3)
        parts.append(ann.drop_ms())
        ann.margins()  # (after the timed call: phx_margins_ms then reports this run's shared part)
        ms = ann.margins_ms()
        rev_parts.append((ms["transpose"], ms["reverse"]))
    bs = ann.batch_sizes()
    n_node, n_edge = bs["n_node"], bs["n_edge"]
    nl = max(int(ann.globals(i).n_limbs) for i in range(n))
    pairs = int(len(rec))
    extra = (n_node + n + 1) * 4 * 5 + n_node * 8 + n_node * nl * 8 * 2 + pairs * (nl * 8 * 2 + 40) + (2 * n + 2) * 8
    med = lambda xs: float(np.median(xs))
    dev = {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    out = {"what": "drop margins call on %d x %d bp, resident" % (n, L), "steps": steps, "phx_run_ms": round(med(run_ms), 4),
           "shared_wall_ms": round(med(rev_ms), 4), "shared_device_ms": {"transpose": round(med([r[0] for r in rev_parts]), 4), "reverse": round(med([r[1] for r in rev_parts]), 4)},
           "drop_wall_ms": round(med(wall_ms), 4), "drop_device_ms": dev, "drop_device_total_ms": round(sum(dev.values()), 4),
           "drop_kernels_ms": round(dev["trees"] + dev["candidates"] + dev["fixups"], 4), "host_ms": round(med(wall_ms) - sum(dev.values()), 4),
           "genes": pairs, "bypass": int(rec["bypass"].sum()), "stats": ann.drop_stats(), "nodes": int(n_node), "edges": int(n_edge), "max_limbs": nl,
           "extra_device_bytes": int(extra)}
    ann.close()
    return out


def trace(outdir, steps, n, L):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "drops", "--", sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--n", str(n), "--len", str(L)]
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
