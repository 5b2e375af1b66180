"""Pinned replacements (phx_pinreplacements_flat) on the golden fixtures: graphs with tRNA nodes, IUPAC letters, bridged runs
and the fixtures' own codon sets, weights and minlen.  Each usable fixture (tests/fixture_draws.py) is one context and one run; per draw of
fixture_draws.draws the draw's refused ORFs and, on every second draw, its biases, with one called gene and one uncalled ORF — the draw's
first required one — required, as tests/test_fixture_sweep_pindrops_gpu.py has it.  Every witness of every solve is weighed edge by edge
from the yardstick's edge list (tests/test_pinreplace_gpu.py::check_records: the required edges it carries, its sum, properties 1, 3 and
4, tRNA pairs among the removed and the added genes), the records of the required ORFs and one more per solve also against their own CuRef
solve; pindrops() stays what it was."""
import pytest

from test_constrain_gpu import run_batch
from test_curate_gpu import DeviceGraph, curate
from test_fixture_sweep_gpu import Yard, indexed
from test_fixture_sweep_host import USABLE
from test_pindrops_gpu import rec_of
from test_pinreplace_gpu import check_records, out_of

import fixture_draws as fd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


@pytest.mark.parametrize("case", USABLE)
def test_every_witness_of_a_fixtures_draws_is_weighed(pa, oracle, case):
    fx = fd.Fixture(case)
    og = fx.graph(oracle)
    assert not fx.error and len(fx.seq) <= fd.MAX_LEN and fd.enough(og), case
    ann = pa.Annotator(pa.make_params(**fx.params))
    try:
        st0, offs0, genes0 = run_batch(ann, [fx.seq], None if fx.trnas is None else [fx.trnas])
        assert st0[0] == 0
        ref = Yard(ann, 0)
        called = ref.called(genes0)
        dg = DeviceGraph(ref, called)
        assert sorted(dg.orf_edge) == sorted(og.orf_edge) and dg.called == og.called, case  # the device's graph is the oracle's
        ok = weighed = exact = gave_up = trna = 0
        for j, d in enumerate(fd.draws(oracle, fx, og)):
            F, R, B = indexed(ref, d)
            gene = next((k for k in called if k not in F), None)
            R = R[:1] + ([gene] if gene is not None else [])
            bias = B if j % 2 == 0 else None  # curate() and constrain() take turns
            st, offs, genes, delta, unmet = curate(ann, [bias], [F], [R]) if bias else ann.constrain([F], [R])
            pd = [x.copy() for x in ann.pindrops()] if j % 2 else None  # (the drops first, without the trees, on every second draw)
            pr = ann.pinreplacements()
            if pd is not None:
                assert [x.tobytes() for x in ann.pindrops()] == [x.tobytes() for x in pd], (case, j)
            pd = ann.pindrops()
            assert int(pr[0][0]) == int(st[0]) and pr[1].tolist() == [0, len(pr[2])] and len(pr[4]) == len(pr[2])
            sol = check_records(ann, ref, F, R, bias, rec_of(pd, 0), out_of(pr, 0), pr[3], limit=1)
            if sol not in ("cycle", None):
                assert sol["bypass"] == int(pr[2]["bypass"].sum()) and (sol["bypass"] == 0 or sol["exact"] >= 1), (case, j)  # no witness went unweighed
                ok += 1
                weighed += sol["bypass"]
                exact += sol["exact"]
                gave_up += sol["gave_up"]
                g = pr[3]
                trna += any(abs(int(f)) == 4 for f in g["frame"])
        print("%s: %d solves with a path, %d witnesses weighed, %d also against their own solve, %d give up a pin, %d solves with a tRNA pair among the removed / added genes"
              % (case, ok, weighed, exact, gave_up, trna))
        assert ok >= 2 and weighed >= 2 and exact >= 2 and gave_up >= 1, (case, ok, weighed, exact, gave_up)
    finally:
        ann.close()
