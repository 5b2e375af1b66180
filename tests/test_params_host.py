"""The -s / -e / -l flags as the test oracle reads them (oracle.make_params) against the product's parser (phx_params_from_flags): both
restate file_handling.py:51-66, where the start codons go into a dict keyed by the lower-case codon (a repeated codon keeps its first
place and its last weight) whose values are divided by the max over the dict.  Every GPU test that hands non-default flags to both sides
relies on the two agreeing, so they are compared here on drawn flag strings.  CPU only."""
import ctypes as C
import random

import pytest

from phanotate_amd import _lib

CODONS = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt"]
MINLENS = (6, 7, 8, 61, 90, 91, 92, 301)


def _case(rnd, c):
    return "".join(x.upper() if rnd.random() < 0.5 else x for x in c) if rnd.random() < 0.3 else c


def _weight(rnd):
    k = rnd.randrange(8)
    if k == 0:
        return "%.*f" % (rnd.randint(1, 6), rnd.uniform(0.001, 1.0))
    if k == 1:
        return "%d%s%d" % (rnd.randint(1, 9), rnd.choice("eE"), -rnd.randint(0, 4))  # 1e-1, 2E-2
    if k == 2:
        return "0"
    if k == 3:
        return "-%.*f" % (rnd.randint(1, 3), rnd.uniform(0.01, 1.0))
    if k == 4:
        return str(rnd.randint(1, 5))  # atg:3,gtg:1: quotients that differ in fp64 and Decimal
    if k == 5:
        return "%.17g" % rnd.uniform(0.001, 2.0)
    return "0.%d" % rnd.randint(1, 999)


def draw_flags(rnd):
    """(start flag, stop flag, minlen): 1 to 16 distinct start codons out of all 64 (so starts that are also stops, starts whose reverse
    complement is a stop, ...), repeated codons, upper case, exponent, zero and negative weights; at least one weight is positive."""
    n = rnd.randint(1, 16)
    cods = rnd.sample(CODONS, n)
    items = [(c, _weight(rnd)) for c in cods]
    for _ in range(rnd.choice([0, 0, 1, 2, 3])):
        if len(items) < 24:
            items.insert(rnd.randrange(len(items) + 1), (rnd.choice(cods), _weight(rnd)))
    last = {}
    for c, w in items:
        last[c] = w
    if not any(float(w) > 0 for w in last.values()):
        c = rnd.choice(cods)
        items.append((c, "%.2f" % rnd.uniform(0.1, 1.0)))
    start = ",".join(_case(rnd, c) + ":" + w for c, w in items)
    stop = ",".join(_case(rnd, c) for c in rnd.sample(CODONS, rnd.randint(1, 5)))
    return start, stop, rnd.choice(MINLENS) if rnd.random() < 0.7 else rnd.randint(6, 500)


def product_params(start, stop, minlen):
    p = _lib.Params()
    rc = _lib.lib().phx_params_from_flags(start.encode(), stop.encode(), minlen, C.byref(p))
    assert rc == 0, (start, stop, minlen, rc)
    return p


def assert_same(o, p, what):
    assert o.minlen == p.minlen, what
    assert o.n_start == p.n_start, what
    assert [o.start[i].value for i in range(o.n_start)] == [p.start[i].value for i in range(p.n_start)], what
    for i in range(o.n_start):
        a, b = o.start_w[i], p.start_w[i]
        assert bytes(C.c_double(a)) == bytes(C.c_double(b)), (what, i, a, b)  # bit for bit (0.0 and -0.0 differ)
    assert o.n_stop == p.n_stop, what
    assert [o.stop[i].value for i in range(o.n_stop)] == [p.stop[i].value for i in range(p.n_stop)], what


def test_oracle_reads_the_flags_like_the_product():
    from oracle import oracle

    rnd = random.Random(20261016)
    n_rep = n_case = n_16 = 0
    for _ in range(600):
        start, stop, minlen = draw_flags(rnd)
        assert_same(oracle.make_params(start, stop, minlen), product_params(start, stop, minlen), (start, stop, minlen))
        cods = [x.split(":")[0].lower() for x in start.split(",")]
        n_rep += len(set(cods)) < len(cods)
        n_case += start != start.lower()
        n_16 += len(set(cods)) == 16
    assert n_rep > 100 and n_case > 100 and n_16 > 10, (n_rep, n_case, n_16)


@pytest.mark.parametrize("start,codons,weights", [
    # the reference keeps the first place and the LAST weight of a repeated codon, and divides by the max over the dict: 0.5 is gone
    ("ATG:0.5,gtg:0.1,atg:1e-1,ttg:2E-2", [b"atg", b"gtg", b"ttg"], [1.0, 1.0, 0.2E-1 / 0.1]),
    ("atg:3,gtg:1,ttg:0.7", [b"atg", b"gtg", b"ttg"], [1.0, 1.0 / 3.0, 0.7 / 3.0]),
    ("gtg:1,atg:0,ttg:-0.5", [b"gtg", b"atg", b"ttg"], [1.0, 0.0, -0.5]),
    ("ttg:0.2,TTG:0.4,Ttg:0.1,atg:0.05", [b"ttg", b"atg"], [1.0, 0.5]),
])
def test_repeated_codons_keep_the_first_place_and_the_last_weight(start, codons, weights):
    from oracle import oracle

    for p in (oracle.make_params(start), product_params(start, "tag,tga,taa", 90)):
        assert [p.start[i].value for i in range(p.n_start)] == codons
        assert [p.start_w[i] for i in range(p.n_start)] == weights


def test_the_oracle_follows_the_reference_dict_on_the_fixture_flags():
    """The raw flags the param_* fixtures were generated with (tests/golden/make_golden.py) give the weights of their normalised text."""
    import numpy as np
    from conftest import golden_cases, golden_params, load_golden
    from oracle import oracle

    n = 0
    for case in golden_cases():
        g, _, _ = load_golden(case)
        if "flags_start" not in g:
            continue
        kw = golden_params(g)
        raw = dict(start_codons=str(g["flags_start"]), stop_codons=str(g["flags_stop"]), minlen=kw["minlen"])
        assert_same(oracle.make_params(**raw), product_params(*raw.values()), case)
        a, b = oracle.make_params(**raw), oracle.make_params(**kw)
        assert [a.start[i].value for i in range(a.n_start)] == [b.start[i].value for i in range(b.n_start)], case
        assert np.allclose([a.start_w[i] for i in range(a.n_start)], [b.start_w[i] for i in range(b.n_start)], rtol=1e-15, atol=0), case
        n += 1
    assert n >= 10, n


def test_flags_the_reference_refuses_are_refused():
    """Every weight 0: the reference divides 0 by 0 (decimal.InvalidOperation); the product refuses the table."""
    p = _lib.Params()
    assert _lib.lib().phx_params_from_flags(b"atg:0,gtg:0", b"tag", 90, C.byref(p)) != 0


def test_flags_beyond_the_products_limits_are_refused_loudly():
    """Flags the reference takes but libphx does not: more than 16 codons, a weight text of 32 characters or more, '_'
    inside a number, a weight beyond fp64.  Refused with an error, never computed on."""
    p = _lib.Params()
    L = _lib.lib()
    seventeen = ",".join("%s:0.5" % c for c in CODONS[:17]).encode()
    for start in (seventeen, b"atg:1,gtg:0.009411764705882352941176470588", b"atg:1,gtg:1_0", b"atg:1e400,gtg:1"):
        assert L.phx_params_from_flags(start, b"tag", 90, C.byref(p)) != 0, start
    with pytest.raises(ValueError):
        from phanotate_amd import api

        api.make_params(seventeen.decode())
