"""Pinned drop margins (phx_pindrops_flat) on the golden fixtures: graphs with tRNA nodes, IUPAC letters, bridged runs and the
fixtures' own codon sets, weights and minlen.  Each usable fixture (tests/fixture_draws.py) is one context and one run; per draw of
fixture_draws.draws the draw's refused ORFs and, on every second draw, its biases, with one called gene and one uncalled ORF — the draw's
first required one — required.  Every record of every solve goes against the yardstick of tests/test_pindrops_gpu.py (check_contig: one
CuRef solve per called gene, integer-exact; a tRNA pair of the path gets no record), and the neighbours of the feature — pinmargins(), the refusal of redrops() — stay as they are."""
import pytest

from test_constrain_gpu import run_batch
from test_curate_gpu import DeviceGraph, curate
from test_fixture_sweep_gpu import Yard, indexed
from test_fixture_sweep_host import USABLE
from test_pindrops_gpu import check_contig, rec_of

import fixture_draws as fd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


@pytest.mark.parametrize("case", USABLE)
def test_every_record_of_a_fixtures_draws_against_the_yardstick(pa, oracle, case):
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
        ok = records = gave_up = trna = 0
        for j, d in enumerate(fd.draws(oracle, fx, og)):
            F, R, B = indexed(ref, d)
            gene = next((k for k in called if k not in F), None)
            R = R[:1] + ([gene] if gene is not None else [])
            bias = B if j % 2 == 0 else None  # curate() and constrain() take turns
            st, offs, genes, delta, unmet = curate(ann, [bias], [F], [R]) if bias else ann.constrain([F], [R])
            pm = [x.tobytes() for x in ann.pinmargins()]
            pd = ann.pindrops()
            assert int(pd[0][0]) == int(st[0]) and pd[1].tolist() == [0, len(pd[2])] and len(pd[3]) == len(pd[2])
            sol = check_contig(ann, ref, F, R, bias, *rec_of(pd, 0), genes)
            if sol not in ("cycle", None):
                assert sol["records"] == len(pd[2]) >= 1, (case, j)  # no record went unchecked
                ok += 1
                records += sol["records"]
                gave_up += sol["gave_up"]
                trna += any(abs(int(f)) == 4 for f in genes["frame"])
            assert [x.tobytes() for x in ann.pinmargins()] == pm, (case, j)
            for refuses in (ann.redrops, ann.rereplacements):
                with pytest.raises(pa.PhxError) as e:
                    refuses()
                assert e.value.code == -13 and "required" in str(e.value), (case, j)
        print("%s: %d solves with a path, %d records, %d give up a pin, %d solves with a tRNA gene on the path" % (case, ok, records, gave_up, trna))
        assert ok >= 2 and records >= 2 and gave_up >= 1, (case, ok, records, gave_up)
    finally:
        ann.close()
