"""The binding's decoders of multi-limb integers (phanotate_amd/api.py: _limbs_to_int, _dist_list) — no GPU and no context.  The expected
values are python-int arithmetic written out here, never a call of the helper under test."""
import numpy as np
import pytest

from phanotate_amd.api import _dist_list, _limbs_to_int

MASK = (1 << 64) - 1


def limbs_of(v, words):
    """words 64-bit limbs of v modulo 2^(64 words), least significant first (two's complement)."""
    v &= (1 << (64 * words)) - 1
    return np.array([(v >> (64 * k)) & MASK for k in range(words)], np.uint64)


@pytest.mark.parametrize("nl", [2, 4, 17])
def test_limbs_to_a_signed_int(nl):
    top = 1 << (64 * nl - 1)
    for v in (0, 1, -1, 12345678901234567890123, -12345678901234567890123, (1 << 64) - 1, 1 << 64, -(1 << 64), -(1 << 64) - 1,
              3 << (64 * (nl - 1)), -(3 << (64 * (nl - 1))) - 7, top - 1, -top):
        got = _limbs_to_int(limbs_of(v, nl), nl)
        assert got == v and isinstance(got, int), (nl, v)
    # a negative value is two's complement across ALL limbs: every limb of -1 is 2^64 - 1, and -2^64 has a zero low limb
    assert limbs_of(-1, nl).tolist() == [MASK] * nl
    assert limbs_of(-(1 << 64), nl).tolist() == [0] + [MASK] * (nl - 1)
    # limbs beyond nl are not read (the path taps hand over 32 words)
    assert _limbs_to_int(np.concatenate([limbs_of(-5, nl), np.array([7, 7], np.uint64)]), nl) == -5


@pytest.mark.parametrize("nl", [2, 4, 17])
def test_distances_and_the_unreached_rule(nl):
    limit = 1 << (64 * nl - 3)  # at or above it: unreached
    winf = 0x7FFFFFFFFFFFFFFF << (64 * (nl - 1))  # the solver's "unreached": top limb 0x7fff..., the others zero
    assert winf >= limit
    vals = [0, 5, -5, limit - 1, limit, limit + 1, winf, -(limit), -(1 << (64 * nl - 1)), 987654321 << 70]
    want = [0, 5, -5, limit - 1, None, None, None, -(limit), -(1 << (64 * nl - 1)), 987654321 << 70]
    rows = np.stack([limbs_of(v, nl) for v in vals])
    assert rows.shape == (len(vals), nl)
    assert _dist_list(rows, nl) == want  # the library reports nl words per node: plain ints
    assert _dist_list(rows[:0], nl) == []


@pytest.mark.parametrize("nl", [2, 4, 17])
def test_pinned_vectors_decode_to_sum_and_count(nl):
    """A contig solved with required ORFs has nl + 1 words per node: x = S - count * 2^(64 nl)."""
    M = 1 << (64 * nl)
    cases = [(S, count) for count in (0, 1, 3) for S in (0, 41, -41, 123456789 << 60, -(123456789 << 60), M // 2 - 1, -(M // 2) + 1)]
    rows = np.stack([limbs_of(S - count * M, nl + 1) for S, count in cases])
    assert rows.shape == (len(cases), nl + 1)
    assert _dist_list(rows, nl) == cases
    # unreached is judged on all nl + 1 words
    winf = 0x7FFFFFFFFFFFFFFF << (64 * nl)
    limit = 1 << (64 * (nl + 1) - 3)
    rows = np.stack([limbs_of(v, nl + 1) for v in (winf, limit)])
    assert _dist_list(rows, nl) == [None, None]
