"""The tie-scratch retry of the re-solves (resolve_attempts, csrc/phx_analyses.inc): the re-annotation and the scenario
batches each own a scratch for the in-order pass that starts at 1 MB.  A solve that wants more reports how much, the scratch grows and the
solve runs again; what comes out must be what one attempt on a large enough scratch gives.  The run's own retry is
test_gpu_parity.py::test_many_ambiguous_contigs_outgrow_the_tie_scratch; the library exposes no counter for a retry, so the tests assert
the condition for one from the kernel's formula: the copies ask for at least twice the initial scratch."""
import numpy as np
import pytest

from ambiguous_contig import TIE_SCRATCH_INITIAL, copies_that_outgrow, large_ambiguous_contig, tie_scratch_need

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


@pytest.fixture(scope="module")
def big():
    found = large_ambiguous_contig()
    assert found is not None, "no large ambiguous contig among the candidates"
    seq, n_node, n_edge = found
    K = copies_that_outgrow(n_node, n_edge)
    assert K * tie_scratch_need(n_node, n_edge) >= 2 * TIE_SCRATCH_INITIAL > (K - 1) * tie_scratch_need(n_node, n_edge)
    return seq, K


def _same_as_run(ann, K, contig_of, st, offs, genes, delta):
    """Entry k of a re-solve's result is the run's device list of contig contig_of(k), with delta 0.0."""
    rst, roffs, rgenes = ann.download_flat(exact=False)
    assert len(st) == K and len(delta) == K and len(offs) == K + 1
    for k in range(K):
        i = contig_of(k)
        assert st[k] == rst[i] == 0 and int(ann.globals(i).tie) == 2
        assert delta[k] == 0.0
        mine, run = genes[offs[k]:offs[k + 1]], rgenes[roffs[i]:roffs[i + 1]]
        assert len(mine) == len(run) > 0 and mine.tobytes() == run.tobytes()


def test_reannotation_outgrows_its_tie_scratch(pa, big):
    """The re-annotation's scratch exists at its initial size after a first call on a small contig without equal-length alternatives;
    K copies of the ambiguous contig, all solved again with nothing refused, then want at least twice that."""
    seq, K = big
    ann = pa.Annotator()
    for seed in range(1, 9):
        (st0, _), = ann.annotate([pa.synth_contig(seed, 6000)])
        if st0 == 0 and int(ann.globals(0).tie) == 0:
            break
    else:
        pytest.fail("no small contig without equal-length alternatives among the seeds")
    ann.reannotate([None], solve_all=True)
    ann.upload([seq] * K)
    ann.run()
    st, offs, genes, delta = ann.reannotate([None] * K, solve_all=True)
    _same_as_run(ann, K, lambda k: k, st, offs, genes, delta)
    ann.close()


def test_scenarios_outgrow_their_tie_scratch(pa, big):
    """K scenarios that refuse nothing of the one ambiguous contig: K slots in one chunk, each with the contig's need."""
    seq, K = big
    ann = pa.Annotator()
    ann.upload([seq])
    ann.run()
    st, offs, genes, delta = ann.scenarios([(0, [])] * K)
    _same_as_run(ann, K, lambda k: 0, st, offs, genes, delta)
    assert ann.scenario_chunks() == 1
    ann.close()
