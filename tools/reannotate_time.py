#!/usr/bin/env python3
"""Cost of a masked re-annotation (phx_reannotate_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/reannotate_time.py [--steps K] [--trace OUTDIR]

One called gene per contig is refused and bit 0 is set, so that all contigs are solved again.  Per step: phx_run (wall), then the
re-annotation (wall; the mask changes from step to step, so that no cached result is handed out), split by the library's HIP events into
mask build, masked solve and in-order parents + path + genes + copies (phx_reannotate_ms).  Next to it, from the same session: the solver
and in-order stages of a context created with `solver_no_wave` (k_sssp_lds as the only solver: the yardstick of §14) and the reverse
pass of phx_margins_ms.  Prints one JSON line.
--trace OUTDIR: afterwards, in a separate child process, `rocprofv3 --kernel-trace --stats` over a few steps, and the stats rows of the
re-annotation's kernels."""
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

KERNELS = ("k_rs_mask", "k_rs_lds", "k_rs_inorder", "k_rs_fin", "k_sssp_lds", "k_inorder")


def measure(steps, n, L):
    import numpy as np

    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, L) for s in range(n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    st, offs, genes = ann.download_flat(exact=False)
    # per contig the ORF indices of its called CDS genes: step k refuses the k-th of them
    called = []
    for i in range(n):
        cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3]
        called.append([ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[: steps + 1]])
    mask_of = lambda k: [[c[k % len(c)]] if c else None for c in called]
    ann.reannotate(mask_of(steps), solve_all=True)  # warm-up: buffers allocated, kernels loaded
    run_ms, wall_ms, parts = [], [], []
    for k in range(steps):
        t0 = time.perf_counter()
        ann.run()
        t1 = time.perf_counter()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not the re-annotation's cost)
        m = mask_of(k)
        t2 = time.perf_counter()
        rst, roffs, rgenes, delta = ann.reannotate(m, solve_all=True)
        t3 = time.perf_counter()
        run_ms.append((t1 - t0) * 1e3)
        wall_ms.append((t3 - t2) * 1e3)
        parts.append(ann.reannotate_ms())
    ann.margins()
    rev = ann.margins_ms()
    bs = ann.batch_sizes()
    nl = max(int(ann.globals(i).n_limbs) for i in range(n))
    ann.close()
    # the yardstick: k_sssp_lds as the only solver, and k_inorder behind it
    ref = pa.Annotator(flags=("solver_no_wave",))
    ref.upload(seqs)
    ref.run()
    ref.set_profiling_stages(["sssp", "inorder"])
    ref.stage_ms()
    ref_run = []
    for _ in range(steps):
        t0 = time.perf_counter()
        ref.run()
        ref_run.append((time.perf_counter() - t0) * 1e3)
    sm = ref.stage_ms()
    ref.close()
    med = lambda xs: float(np.median(xs))
    dev = {k: round(med([p[k] for p in parts]), 4) for k in parts[0]}
    sssp = sm["sssp"][0] / steps
    ino = sm["inorder"][0] / steps
    bound = 1.15 * (sssp + ino)
    out = {"what": "re-annotation of %d x %d bp, resident, one called gene per contig refused, every contig solved again" % (n, L), "steps": steps,
           "phx_run_ms": round(med(run_ms), 4), "reannotate_wall_ms": round(med(wall_ms), 4), "reannotate_device_ms": dev,
           "reannotate_device_total_ms": round(sum(dev.values()), 4), "reannotate_kernels_ms": round(dev["mask"] + dev["solve"], 4),
           "no_wave_sssp_stage_ms": round(sssp, 4), "no_wave_inorder_stage_ms": round(ino, 4), "no_wave_run_ms": round(med(ref_run), 4),
           "bound_ms": round(bound, 4), "margins_reverse_ms": round(rev["reverse"], 4),
           "genes": int(len(rgenes)), "no_path": int((rst == 1).sum()), "delta_max": float(np.max(delta[np.isfinite(delta)])) if np.isfinite(delta).any() else None,
           "nodes": int(bs["n_node"]), "edges": int(bs["n_edge"]), "max_limbs": nl}
    return out


def trace(outdir, steps, n, L):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "reannotate", "--", sys.executable, os.path.abspath(__file__), "--steps", str(steps), "--n", str(n), "--len", str(L)]
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
