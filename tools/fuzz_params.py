#!/usr/bin/env python3
"""tools/fuzz_gpu.py's contigs under OTHER flags than the defaults: start codon sets and weights (-s), stop codon sets (-e), minimum
ORF lengths (-l) drawn per batch of 60 contigs; libphx (with the certificate and the host re-solve on) against the oracle run with the
same flags.  A contig on which the two disagree while the library says it solved it again on the host is decided by python's decimal
(dump.python_resolve), as in fuzz_gpu.py.  Run on the GPU box:
    python tools/fuzz_params.py [n_batches] [seed]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from concurrent.futures import ProcessPoolExecutor
import numpy as np
from fuzz_gpu import make

CODONS = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt"]
RC = lambda c: c[::-1].translate(str.maketrans("acgt", "tgca"))

def draw_flags(rng):
    """One flag set: 1 to 16 start codons, some that are also stops or whose reverse complement is a stop (the elif chain of
    functions.py:198-215), sometimes without atg; repeated codons (dict semantics: first place, last weight), upper case, exponent,
    zero and negative weights (at least one positive); 1 to 4 stops, sometimes reverse complements of each other; minlen around the
    multiples of 3."""
    stops = list(rng.choice(["tag", "tga", "taa", "cta", "tca", "tta", "ttg"], int(rng.randint(1, 5)), replace=False))
    if rng.rand() < 0.15: stops.append(RC(stops[0]))
    k = int(rng.choice([1, 2, 3, 3, 4, 6, 9, 16]))
    pool = ["gtg", "ttg", "ctg", "att", "ata"] + [c for c in CODONS if c not in ("atg", "gtg", "ttg", "ctg", "att", "ata")]
    odd = [c for c in CODONS if c in stops or RC(c) in stops]  # codons that fall into two classes
    cs = [] if rng.rand() < 0.15 else ["atg"]
    if rng.rand() < 0.4: cs.append(str(rng.choice(odd)))
    while len(cs) < k:
        c = str(rng.choice(pool[:5] if rng.rand() < 0.5 else pool))
        if c not in cs: cs.append(c)
    def weight():
        f = rng.randint(10)
        if f == 0: return "%d%s%d" % (rng.randint(1, 10), "eE"[rng.randint(2)], -rng.randint(0, 4))
        if f == 1: return "0"
        if f == 2: return "-0.%02d" % rng.randint(1, 100)
        if f == 3: return str(rng.randint(1, 4))
        nd = int(rng.choice([1, 2, 3, 6]))
        return ("%." + str(nd) + "f") % max(round(float(rng.uniform(0.01, 1.0)), nd), 10.0 ** -nd)
    items = [[c, weight()] for c in cs]
    if rng.rand() < 0.3: items[0][1] = "1"
    for _ in range(int(rng.choice([0, 0, 1, 2]))):  # a repeated codon
        items.insert(int(rng.randint(len(items) + 1)), [str(rng.choice(cs)), weight()])
    last = {}
    for c, w in items: last[c] = w
    if not any(float(w) > 0 for w in last.values()): items.append([cs[0], "0.5"])
    up = lambda c: c.upper() if rng.rand() < 0.2 else c
    return dict(start_codons=",".join(up(c) + ":" + w for c, w in items), stop_codons=",".join(up(c) for c in stops),
                minlen=int(rng.choice([6, 7, 8, 61, 90, 91, 92, 301])))

def orc(arg):
    seq, kw = arg
    from oracle import oracle
    o = oracle.run(seq, oracle.make_params(**kw))
    if o["status"] < 0:
        return int(o["status"]), ([], [], [])
    return 0, (np.asarray(o["gene_left"]).tolist(), np.asarray(o["gene_right"]).tolist(), np.asarray(o["gene_strand"]).tolist())

def main():
    nb = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    rng = np.random.RandomState(seed)
    import phanotate_amd as pa
    import os as _os, sys as _sys
    _sys.path.insert(0, _os.path.join(_os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))), "tests"))
    import decimal_replay as dump
    bad = n = n_host = exact_wins = 0
    with ProcessPoolExecutor(max_workers=min(32, os.cpu_count() or 1)) as ex:
        for b in range(nb):
            kw = draw_flags(rng)
            seqs = [make(rng) for _ in range(60)]
            want = list(ex.map(orc, [(s, kw) for s in seqs], chunksize=4))
            ann = pa.Annotator(pa.make_params(**kw))
            res = ann.annotate(seqs)
            cert = ann.certified()
            n_host += int((cert == 2).sum())
            for i, (status, genes) in enumerate(res):
                st, exp = want[i]
                n += 1
                ok = (status == st) if st < 0 else (status >= 0 and [int(x) for x in genes["left"]] == exp[0] and [int(x) for x in genes["right"]] == exp[1] and [int(x) for x in genes["strand"]] == exp[2])
                if not ok and cert[i] == 2:
                    py = dump.python_resolve(ann, i, seqs[i], kw["start_codons"])
                    if [(int(x["left"]), int(x["right"]), int(x["strand"])) for x in genes] == [t[:3] for t in py]:
                        exact_wins += 1
                        continue
                if not ok:
                    bad += 1
                    if bad <= 5: print("MISMATCH batch %d contig %d (len %d) flags %s: status %d vs %d, %d vs %d genes, cert %d" % (b, i, len(seqs[i]), kw, status, st, len(genes), len(exp[0]), cert[i]))
            ann.close()
    print("fuzz_params seed %d: %d contigs in %d batches of their own flags, %d mismatches; solved again on the host %d (of which decimal.Decimal sides with the library against the fp64 oracle: %d)" % (seed, n, nb, bad, n_host, exact_wins))
    return 1 if bad else 0

if __name__ == "__main__":
    sys.exit(main())
