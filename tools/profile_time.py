#!/usr/bin/env python3
"""Cost of the coding profiles (phx_profile_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/profile_time.py [--steps K] [--trace OUTDIR]

Per step: phx_run (wall), the margins' shared part through the first margins call (its reverse-pass time is the profile's allowance:
the profile touches each edge once per track, the reverse pass several times), then the first profile call after it (wall), split by the
library's HIP events into the tables (k_pf_cand: candidates, tables, push-down), the records (k_pf_rec) and their copy to the host.
Prints one JSON line, with the extra device memory of the pass.  --trace OUTDIR: afterwards, in a separate child process,
`rocprofv3 --kernel-trace --stats` over a few steps, and the stats rows of the new kernels."""
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

KERNELS = ("k_pf_cand", "k_pf_rec", "k_sssp_rev")
TAB_LDS = 4096  # PF_TAB_LDS


def cells(n):
    return n * n.bit_length()  # n (floor(log2 n) + 1)


def measure(steps, n, L):
    import numpy as np

    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, L) for s in range(n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    ann.download_flat()
    ann.margins()
    ann.profile()  # warm-up: buffers of the pass allocated, kernels loaded
    run_ms, wall_ms, parts, rev = [], [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        ann.run()
        t1 = time.perf_counter()
        ann.margins()  # (the shared part — out-edge CSR, reverse pass — is not part of the profile's cost; its reverse pass is the allowance)
        rev.append(ann.margins_ms()["reverse"])
        t2 = time.perf_counter()
        st, offs, rec = ann.profile()
        t3 = time.perf_counter()
        run_ms.append((t1 - t0) * 1e3)
        wall_ms.append((t3 - t2) * 1e3)
        parts.append(ann.profile_ms())
    slots = [int(ann.globals(i).n_node) - 1 for i in range(n) if st[i] >= 0 and ann.globals(i).n_node > 2]
    table = sum(cells(s) for s in slots if cells(s) > TAB_LDS) * 8
    extra = table + sum(slots) * 32 + (2 * n + 2) * 8
    med = lambda xs: float(np.median(xs))
    dev = {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    out = {"what": "profile call on %d x %d bp, resident" % (n, L), "steps": steps, "phx_run_ms": round(med(run_ms), 4), "profile_wall_ms": round(med(wall_ms), 4),
           "profile_device_ms": dev, "profile_kernels_ms": round(dev["tables"] + dev["records"], 4), "allowance_reverse_pass_ms": round(med(rev), 4),
           "host_ms": round(med(wall_ms) - sum(dev.values()), 4), "slots": int(sum(slots)), "contigs_in_global_memory": sum(1 for s in slots if cells(s) > TAB_LDS),
           "table_bytes": int(table), "extra_device_bytes": int(extra)}
    ann.close()
    return out


def trace(outdir, steps, n, L):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "profile", "--", sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--n", str(n), "--len", str(L)]
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
