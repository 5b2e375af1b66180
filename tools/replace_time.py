#!/usr/bin/env python3
"""Cost of the drop replacements (phx_replacements_flat) on the bench batch: 1000 synthetic 50 kb contigs, resident.

    python tools/replace_time.py [--steps K]

Per step: phx_run, then the first replacements call after it (wall), which computes the drop margins first (with the one-hop trees kept,
phx_drop_ms) and then the replacement stage, split by the library's HIP events into argmin (k_rp_pick, k_rp_cross), walk + genes
(k_rp_walk twice, with the offsets between) and the copy to the host.  Prints one JSON line with medians, the counts and the extra
device memory.  For per-kernel figures run it under `rocprofv3 --kernel-trace --stats -- python tools/replace_time.py`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    import phanotate_amd as pa

    seqs = [pa.synth_contig(s, a.len) for s in range(a.n)]
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    ann.download_flat()
    ann.replacements()  # warm-up
    wall, drop, repl = [], [], []
    for _ in range(a.steps):
        ann.run()
        ann.download_flat()
        t0 = time.perf_counter()
        st, offs, rec, genes = ann.replacements()
        wall.append((time.perf_counter() - t0) * 1e3)
        drop.append(ann.drop_ms())
        repl.append(ann.replacements_ms())
    med = lambda xs: round(statistics.median(xs), 3)
    R = len(rec)
    print(json.dumps({"contigs": a.n, "bases": a.n * a.len, "records": R, "with_bypass": int(rec["bypass"].sum()), "genes": int(len(genes)),
                      "wall_ms": med(wall), "drop_ms": {k: med([d[k] for d in drop]) for k in drop[0]},
                      "replacement_ms": {k: med([d[k] for d in repl]) for k in repl[0]},
                      "replacement_device_ms": med([sum(d.values()) - d["download"] for d in repl]), "added_genes": int(rec["n_added"].sum()),
                      "drop_stats": ann.drop_stats()}))
    ann.close()


if __name__ == "__main__":
    main()
