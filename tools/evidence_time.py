#!/usr/bin/env python3
"""Cost of an evidence-weighted re-annotation (phx_evidence_flat) next to the masked one (§14), same session.

    python tools/evidence_time.py [--steps K] [--n N] [--len L]

Three measurements, one JSON line each (medians over the steps in the first two):

  batch   N synthetic contigs of L bp, resident (default: the bench batch, 1000 x 50 kb).  Per step one uncalled ORF per contig gets a
          bonus of 2.5 SCORE units (another ORF every step, so that no cached result is handed out) and every contig is solved again
          under the bias policy (k_rs_mask, k_rs_lds, k_rs_inorder); then, as tools/reannotate_time.py does, one called gene per contig is
          refused and every contig solved again under the masked policy (k_rs_lds).  Device times by the library's HIP events
          (phx_reannotate_ms serves both): mask, solve, finish.  bound_ms = the sibling's solve time plus 15 %.
  lone    the same two questions on the Lambda contig alone (tests/golden/NC_001416.1).
  cycle   Lambda alone, one ORF at a time with a bonus of a million SCORE units, far beyond every cycle's length: the solve time of the
          calls that end as PHX_S_NEGCYCLE (the sweep's caps find the cycle) next to the calls that settle."""
import argparse
import gzip
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(what, seqs, steps):
    import numpy as np

    import phanotate_amd as pa

    n = len(seqs)
    ann = pa.Annotator()
    ann.upload(seqs)
    ann.run()
    st, offs, genes = ann.download_flat(exact=False)
    called, others = [], []
    oo = ann.orf_offsets()
    for i in range(n):
        cds = [g for g in genes[offs[i]:offs[i + 1]] if abs(int(g["frame"])) <= 3]
        c = [ann.orf_index(i, int(g["left"]), int(g["right"]), int(g["strand"])) for g in cds[: steps + 1]] if st[i] == 0 else []
        called.append(c)
        n_orf = int(oo[i + 1] - oo[i])
        others.append([k for k in range(min(n_orf, 4 * steps + 8)) if k not in c][: steps + 1])  # (ORFs in orfs(i) order: the contig's left end)
    mask_of = lambda k: [[c[k % len(c)]] if c else None for c in called]
    bias_of = lambda k: [[(o[k % len(o)], -2.5)] if o else None for o in others]
    ann.reannotate(mask_of(steps), solve_all=True)  # warm-up: buffers allocated, kernels loaded
    ann.evidence(bias_of(steps), solve_all=True)
    ev, rs, ev_wall, rs_wall = [], [], [], []
    status = delta = None
    for k in range(steps):
        ann.run()
        ann.orf_offsets()  # (the taps behind it, the certificate among them, are not the re-annotation's cost)
        b, m = bias_of(k), mask_of(k)
        t0 = time.perf_counter()
        status, _, _, delta = ann.evidence(b, solve_all=True)
        t1 = time.perf_counter()
        ev.append(ann.reannotate_ms())
        t2 = time.perf_counter()
        ann.reannotate(m, solve_all=True)
        t3 = time.perf_counter()
        rs.append(ann.reannotate_ms())
        ev_wall.append((t1 - t0) * 1e3)
        rs_wall.append((t3 - t2) * 1e3)
    bs = ann.batch_sizes()
    ann.close()
    med = lambda xs: float(np.median(xs))
    e = {k: round(med([p[k] for p in ev]), 4) for k in ev[0]}
    r = {k: round(med([p[k] for p in rs]), 4) for k in rs[0]}
    fin = np.isfinite(delta)
    return {"what": what, "steps": steps, "evidence_device_ms": e, "reannotate_device_ms": r, "evidence_wall_ms": round(med(ev_wall), 4), "reannotate_wall_ms": round(med(rs_wall), 4),
            "bound_ms": round(1.15 * r["solve"], 4), "within_bound": bool(e["solve"] <= 1.15 * r["solve"]), "solve_ratio": round(e["solve"] / r["solve"], 4) if r["solve"] else None,
            "negcycle": int((status == -9).sum()), "moved": int((delta[fin] < 0).sum()), "nodes": int(bs["n_node"]), "edges": int(bs["n_edge"]),
            "bias_words_bytes": 8 * int(bs["n_edge"]), "bias_bitmap_bytes": int(bs["n_edge"]) // 8}


def cycles(seq, tries):
    import numpy as np

    import phanotate_amd as pa

    ann = pa.Annotator()
    ann.upload([seq])
    ann.run()
    n_orf = int(ann.orf_offsets()[1])
    ann.evidence([[(0, -1.0)]])  # warm-up
    neg, ok = [], []
    for k in np.random.RandomState(19).choice(n_orf, min(tries, n_orf), replace=False).tolist():
        status = ann.evidence([[(k, -1e6)]])[0]
        (neg if status[0] == -9 else ok).append(ann.reannotate_ms()["solve"])
    V = int(ann.globals(0).n_node)
    ann.close()
    f = lambda xs: {"n": len(xs), "median_ms": round(float(np.median(xs)), 4), "max_ms": round(float(np.max(xs)), 4)} if xs else {"n": 0}
    return {"what": "cycle: Lambda, one ORF at a time with a bonus of 1e6 SCORE units", "nodes": V, "negcycle_solve": f(neg), "settled_solve": f(ok)}


def main():
    import phanotate_amd as pa

    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--len", type=int, default=50000)
    a = ap.parse_args()
    print(json.dumps(measure("batch: %d x %d bp, one ORF per contig biased / one called gene per contig refused, every contig solved again" % (a.n, a.len),
                             [pa.synth_contig(s, a.len) for s in range(a.n)], a.steps)), flush=True)
    with gzip.open(os.path.join(ROOT, "tests", "golden", "NC_001416.1.fasta.gz"), "rt") as f:
        lam = "".join(f.read().split("\n")[1:])
    print(json.dumps(measure("lone: Lambda, one ORF biased / one called gene refused", [lam], a.steps)), flush=True)
    print(json.dumps(cycles(lam, 200)), flush=True)


if __name__ == "__main__":
    main()
