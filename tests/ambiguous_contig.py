"""The large ambiguous contig of the tie-scratch tests, searched once per test session.

The in-order pass (k_inorder, and k_rs_inorder / k_sc_inorder of the re-solves: one body, phx_inorder.inc) bump-allocates, for every contig
with equal-length alternative paths, 8 B + 7 x 4 B per node and 12 B per edge from a scratch buffer that every one of its three owners — the
run, the re-annotation, the scenario batches — starts at 1 MB and grows when a solve reports that it wanted more."""
import functools
import os
import sys

import numpy as np

from conftest import ROOT

TIE_SCRATCH_INITIAL = 1 << 20  # bytes: max(the largest need a run of the context reported, 1 MB), while the owner has no buffer yet


@functools.lru_cache(maxsize=None)
def large_ambiguous_contig():
    """(sequence, n_node, n_edge) of the first fuzz contig of seed 101 that the device solves with status 0, resolves a tie on
    (globals(i).tie == 2) and that has more than 1500 nodes; None when the 300 candidates hold none."""
    import phanotate_amd as pa

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fuzz_gpu

    rng = np.random.RandomState(101)
    cands = [fuzz_gpu.make(rng) for _ in range(300)]
    ann = pa.Annotator()
    try:
        for b0 in range(0, 300, 100):
            res = ann.annotate(cands[b0 : b0 + 100])
            for i, (st, genes) in enumerate(res):
                g = ann.globals(i)
                if st == 0 and g.tie == 2 and g.n_node > 1500:
                    return cands[b0 + i], int(g.n_node), int(g.n_edge)
    finally:
        ann.close()
    return None


def tie_scratch_need(n_node, n_edge):
    """Bytes one copy of a contig with equal-length alternatives takes from the scratch (a lower bound: the kernel rounds each part up)."""
    return 36 * n_node + 12 * n_edge


def copies_that_outgrow(n_node, n_edge):
    """The smallest number of copies whose summed need is at least twice the initial scratch."""
    return -(-2 * TIE_SCRATCH_INITIAL // tie_scratch_need(n_node, n_edge))
