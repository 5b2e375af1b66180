"""Coding profiles on the golden fixtures tests/test_profile_gpu.py does not check value for value — Lambda and T4, the
other 50 kb synthetics, the tRNA fixtures on them: the invariants of test_profile_gpu.check_invariants.  One context and one run per
fixture, under its own params and tRNAs."""
import pytest

from conftest import golden_cases
from test_profile_gpu import FULL_CASES, annotate, check_invariants

pytestmark = pytest.mark.gpu

REST = [c for c in golden_cases() if c not in FULL_CASES]


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


def test_the_sweep_covers_what_is_left():
    assert {"NC_001416.1", "NC_000866.1", "trna_lambda", "trna_synth6k"} <= set(REST) and len(REST) >= 10
    assert sorted(REST + FULL_CASES) == golden_cases()


@pytest.mark.parametrize("case", REST)
def test_invariants(pa, case):
    ann, L, st, rec, mrec = annotate(pa, case)
    assert st == 0, case  # (every fixture left for the sweep has a path)
    check_invariants(ann, 0, L, st, rec, mrec)
    ann.close()
