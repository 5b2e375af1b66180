"""k_graph_chain (nodes, node attributes, edge count and scan of a contig in one launch) and the o-term split (k_node_attr names the ORF,
k_node_oterm reads its p_stop behind k_orf_stats) against the staged kernels on the same stream layout (flags=("no_chain",)): statuses,
node / ORF / edge tables, paths, distances and gene records byte for byte, and the same again on a second run of each context."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

# stops of both strands in every frame every 12 bp: no ORF, so no node but source and target ('taa' * 100 has five ORFs: its other frames are open)
NO_ORF = b"ttaactagctaa" * 25
ONE_ORF = NO_ORF[:60] + b"atg" + b"gctgaa" * 20 + NO_ORF[60:]  # one start, 40 sense codons, the background's next stop


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def _snapshot(a, n, sample):
    st, offs, genes = a.download_flat()
    taps = {}
    for i in sample:
        gl = a.globals(i)
        t = [int(st[i]), gl.n_orf, gl.n_node, gl.n_edge]
        if st[i] >= 0 and gl.n_node > 2:
            nd, ed = a.nodes(i), a.edges(i)
            # a tRNA node has no o-term: nothing writes its slot, so it is left out of the comparison (such a node's reference rank lies
            # behind the CDS nodes' and in front of the source's)
            trna = (nd["refidx"] >= gl.n_orf + gl.n_group) & (np.arange(len(nd)) < gl.n_node - 2)
            nd["o"][trna] = 0.0
            p, d = a.path(i)
            t += [nd.tobytes(), nd["other"].tobytes(), nd["o"].tobytes(), a.orfs(i).tobytes(), ed.tobytes(), p.tobytes(), d, a.dist(i)]
        taps[i] = t
    return dict(status=st.tobytes(), offs=offs.tobytes(), genes=genes.tobytes(), taps=taps, n_genes=int(offs[-1]), chain_runs=a.chain_runs())


def _run_twice(pa, seqs, flags, sample, hits=None):
    a = pa.Annotator(flags=flags)
    a.upload(seqs)
    if hits is not None:
        a.set_trnas(hits)
    a.run()  # (sizes the buffers: the staged kernels)
    a.run()
    first = _snapshot(a, len(seqs), sample)
    a.run()
    second = _snapshot(a, len(seqs), sample)
    a.close()
    return first, second


def _same(x, y, what):
    for k in ("status", "offs", "genes"):
        assert x[k] == y[k], (what, k)
    for i in x["taps"]:
        assert x["taps"][i] == y["taps"][i], (what, "contig", i)


def _check(pa, seqs, sample, hits=None, chained=True):
    d1, d2 = _run_twice(pa, seqs, (), sample, hits)
    s1, s2 = _run_twice(pa, seqs, ("no_chain",), sample, hits)
    # the run that sizes the buffers is staged; the two after it are k_graph_chain's in the default context (a few long contigs: never)
    assert (d1["chain_runs"], d2["chain_runs"]) == ((1, 2) if chained else (0, 0))
    assert (s1["chain_runs"], s2["chain_runs"]) == (0, 0)
    _same(d1, d2, "default context, second run")
    _same(s1, s2, "no_chain context, second run")
    _same(d1, s1, "default against no_chain")
    return d1


def _mixed(pa):
    lam = load_golden("NC_001416.1")[2].lower().encode()
    # (an all-n contig is legal input — the reference gives it status 0 and six ORFs —, so a bad-letter contig stands beside it for the negative status)
    return [b"n" * 400, NO_ORF, ONE_ORF, lam, pa.synth_contig(7, 100000), b"acgtnnacgx" * 40]


def test_640_contigs_large_batch_streams(pa):
    seqs = [pa.synth_contig(91000 + i, 3000) for i in range(640)]
    got = _check(pa, seqs, [0, 1, 319, 638, 639])
    assert got["n_genes"] > 0


def test_1100_contigs_two_pass_layout(pa):
    seqs = [pa.synth_contig(92000 + i, 1500) for i in range(1100)]
    _check(pa, seqs, [0, 1023, 1024, 1025, 1099])


def test_mixed_batch(pa):
    seqs = _mixed(pa)
    got = _check(pa, seqs, range(len(seqs)))
    t = got["taps"]
    assert t[5][0] < 0                        # a letter outside the alphabet: an error status
    assert t[1][1] == 0 and t[1][2] <= 2      # no ORF: source and target at most
    assert t[2][1] == 1                       # exactly one ORF
    assert t[4][2] > 4096                     # the scan's LDS segment carries over


def test_mixed_batch_genes_equal_the_oracle(pa, oracle):
    seqs = _mixed(pa)
    a = pa.Annotator()
    a.upload(seqs)
    a.run()
    a.run()
    st, offs, genes = a.download_flat()
    a.close()
    for i, s in enumerate(seqs):
        ref = oracle.run(s)
        assert int(st[i]) == int(ref["status"]), i
        if ref["status"] < 0:
            continue
        g = genes[offs[i]:offs[i + 1]]
        assert np.array_equal(g["left"], ref["gene_left"]) and np.array_equal(g["right"], ref["gene_right"]), i
        assert np.array_equal(g["strand"], ref["gene_strand"].astype(np.int32)), i
        np.testing.assert_allclose(g["score"], ref["gene_score"], rtol=1e-6)


def test_t4_alone_staged_nodes(pa):
    """A lone long contig keeps the staged node kernels in both contexts: only the o-term split is under test."""
    t4 = load_golden("NC_000866.1")[2].lower().encode()
    _check(pa, [t4], [0], chained=False)


def test_batch_with_trna_hits(pa):
    rng = np.random.RandomState(8)
    seqs = [pa.synth_contig(3500 + i, int(rng.choice([600, 3000, 20000, 40000]))) for i in range(33)]
    seqs[3] = b"acgtnnacgx" * 50
    seqs[1] = b"acgta"
    hits = [[(100, 180), (400, 320)] if (i % 3 == 0 and len(s) > 1000) else [] for i, s in enumerate(seqs)]
    _check(pa, seqs, [0, 1, 3, 6, 16, 30, 32], hits)


def test_context_reuse(pa):
    A = [pa.synth_contig(93000 + i, 3000 + 200 * (i % 5)) for i in range(40)]
    B = [pa.synth_contig(94000 + i, 6000) for i in range(700)]
    sample = [0, 7, 39]
    fresh, _ = _run_twice(pa, A, (), sample)
    for flags in ((), ("no_chain",)):
        a = pa.Annotator(flags=flags)
        for batch in (A, B, A):
            a.upload(batch)
            a.run()
            a.run()
        again = _snapshot(a, len(A), sample)
        a.close()
        _same(fresh, again, "A after B on one context, flags %r" % (flags,))
