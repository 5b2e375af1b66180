"""The device under other -s / -e / -l flags than the reference's defaults (file_handling.py:51-66).  The codon tables decide which
k_features runs (the default classes take k_features<false,true>, every other table the cls_tab one), how the elif chain of
functions.py:198-215 classes a codon that is in two of its sets, which ORFs train the GC frame plot when atg is no start
(functions.py:186-190, 241-242, 266) and where dmin = (minlen - 1) / 3 cuts.  Every flag set goes in as the user writes it (the raw flag
text: repeated codons, upper case, exponents, zero and negative weights), on the product and on the oracle alike
(tests/test_params_host.py holds the two parsers together), through multi-contig batches, k_front, the segment solvers, the side
streams of large batches, the create flags, the certificate, margins, drops and the CLI."""
import os
import subprocess
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_cases, load_golden

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

CODONS = [a + b + c for a in "acgt" for b in "acgt" for c in "acgt"]
PARAM_CASES = [c for c in golden_cases() if c.startswith("param_")]
# one non-default table for the kernel paths: a stop whose reverse complement is a stop (cta), a repeated codon, upper case, exponents,
# minlen not a multiple of 3.  (Not start_rc_stop: its rc-start codons make every 60 kb contig dense — no wavefront kernel, so no segments.)
KP = dict(start_codons="ATG:0.5,gtg:0.1,atg:1e-1,ttg:2E-2", stop_codons="tag,cta,taa", minlen=91)


@pytest.fixture(scope="module")
def pa():
    import phanotate_amd

    return phanotate_amd


@pytest.fixture(scope="module")
def pool():
    import multiprocessing

    # the oracle on CPU workers; spawned (not forked from a process that holds the GPU), they never open the device
    with ProcessPoolExecutor(max_workers=8, mp_context=multiprocessing.get_context("spawn")) as ex:
        yield ex


def rc(c):
    return c[::-1].translate(str.maketrans("acgt", "tgca"))


def raw_flags(g):
    return dict(start_codons=str(g["flags_start"]), stop_codons=str(g["flags_stop"]), minlen=int(g["params_minlen"]))


def lowered(kw):
    """The codon lists as test_gpu_parity.check_contig reads them (lower case; a repeated codon is harmless there)."""
    return dict(kw, start_codons=kw["start_codons"].lower(), stop_codons=kw["stop_codons"].lower())


def codon_sets(kw):
    return [x.split(":")[0] for x in kw["start_codons"].lower().split(",")], kw["stop_codons"].lower().split(",")


def fuzz(seed, n):
    import fuzz_gpu

    rng = np.random.RandomState(seed)
    return [fuzz_gpu.make(rng) for _ in range(n)]


def edge_contigs(pa, kw, seed):
    """Contigs built on the flag set's own codons: (a) a soup of its starts, stops and their reverse complements in every frame; (b) the
    contig-end fragments (pseudo starts) as long ORFs of both strands that begin with atg, around an ordinary stretch; (c) ORFs of
    minlen - 1, minlen and minlen + 1 bases between random flanks."""
    rng = np.random.RandomState(seed)
    starts, stops = codon_sets(kw)
    special = starts + [rc(c) for c in starts] + stops + [rc(c) for c in stops]
    free = [c for c in CODONS if c not in stops]  # no stop of this table in frame
    soup = "".join(rng.choice(special + CODONS, 1500))
    body = lambda n: "".join(rng.choice(free, n))
    ends = "atg" + body(150) + pa.synth_contig(seed, 1500).decode() + rc("atg" + body(150))
    m = kw["minlen"]
    parts = []
    for ln in (m - 1, m, m + 1):  # start codon + k codons + stop = 3k + 6 bases; lengths that are no multiple of 3 fall between two
        k = max(0, (ln - 6 + 2) // 3)
        parts.append("".join(rng.choice(CODONS, 60)) + str(rng.choice(starts)) + body(k) + stops[0])
    near = "".join(parts) + "".join(rng.choice(CODONS, 60))
    return [soup, ends, near]


def orc(arg):
    seq, kw = arg
    from oracle import oracle

    return oracle.run(seq, oracle.make_params(**kw))


def genes_of(o):
    return list(zip(o["gene_left"].tolist(), o["gene_right"].tolist(), o["gene_strand"].tolist()))


def flat_genes(g):
    return list(zip(g["left"].tolist(), g["right"].tolist(), g["strand"].tolist()))


def compare(ann, seqs, kw, st, offs, genes, want):
    """The fuzz rule (tools/fuzz_gpu.py, fuzz_params.py): status and genes equal the oracle's; a contig may differ only where the library
    solved it again on the reference's integers (certified() == 2) and Python's decimal (decimal_replay.python_resolve) agrees with it.
    Returns (compared, decided by decimal, beyond the oracle's fp64) counts and the indices that equal the oracle."""
    import decimal_replay as dump

    cert = ann.certified()
    n = by_dec = beyond = 0
    same = []
    for i, o in enumerate(want):
        g = genes[offs[i]:offs[i + 1]]
        if o["status"] == -7 and st[i] == 0:  # an ORF weight beyond fp64: the oracle gives up, the library solves it on the host
            assert cert[i] == 2 and len(g) > 0, i
            beyond += 1
            continue
        n += 1
        if o["status"] < 0:
            assert st[i] == o["status"] and len(g) == 0, (i, st[i], o["status"], kw)
            continue
        assert st[i] >= 0, (i, st[i], kw)
        if flat_genes(g) == genes_of(o):
            same.append(i)
            continue
        assert cert[i] == 2, (i, len(seqs[i]), kw, len(g), len(o["gene_left"]))
        py = dump.python_resolve(ann, i, seqs[i], kw["start_codons"])
        assert [(int(x["left"]), int(x["right"]), int(x["strand"])) for x in g] == [t[:3] for t in py], (i, kw)
        by_dec += 1
    return n, by_dec, beyond, same


def run3(ann, seqs):
    """Upload and run three times (the first run sizes the buffers, the third replays the captured graph): the same bytes every time."""
    ann.upload(seqs)
    out = None
    for r in range(3):
        ann.run()
        st, offs, genes = ann.download_flat()
        b = (st.tobytes(), offs.tobytes(), genes.tobytes())
        assert out is None or b == out[3], r
        out = (st, offs, genes, b)
    return out[:3]


@pytest.mark.parametrize("case", PARAM_CASES)
def test_flag_set_batch(case, pa, oracle, pool):
    """The fixture contig, 40 fuzz contigs and 3 contigs built on the flag set's codons in one batch, with the raw flags: every status and
    gene list against the oracle, all the stage taps on a sample, the fixture's own contig equal to the reference's genes."""
    from test_gpu_parity import check_contig

    g, name, seq = load_golden(case)
    kw = raw_flags(g)
    k = PARAM_CASES.index(case)
    seqs = [seq] + fuzz(700 + k, 40) + edge_contigs(pa, kw, 800 + k)
    ann = pa.Annotator(pa.make_params(**kw))
    st, offs, genes = run3(ann, seqs)
    want = list(pool.map(orc, [(s, kw) for s in seqs], chunksize=2))
    n, by_dec, beyond, same = compare(ann, seqs, kw, st, offs, genes, want)
    assert n >= 40 and 0 in same, (n, by_dec, beyond)
    g0 = genes[offs[0]:offs[1]]
    assert np.array_equal(g0["left"], g["gene_left"]) and np.array_equal(g0["right"], g["gene_right"])
    assert np.array_equal(g0["strand"], g["gene_strand"].astype(np.int32)) and np.array_equal(g0["frame"], g["gene_frame"].astype(np.int32))
    if len(g0):
        np.testing.assert_allclose(g0["score"], g["gene_score"], rtol=1e-6)
    rng = np.random.RandomState(k)
    fz = [i for i in same if 1 <= i <= 40 and len(seqs[i]) <= 12000]
    sample = [0] + [i for i in same if i > 40] + sorted(rng.choice(fz, min(3, len(fz)), replace=False).tolist())
    for i in sample:
        check_contig(ann, i, seqs[i], want[i], genes[offs[i]:offs[i + 1]], int(st[i]), lowered(kw))
    ann.close()


def test_kernel_paths_under_one_non_default_table(pa, oracle, pool):
    """KP (cta both a stop and the reverse complement of one, a repeated codon, minlen 91) through the segment solvers (a lone 60 kb contig), k_front (batches of
    1 to 4 contigs), the side streams (720 contigs) and the create flags that switch kernels off: the oracle's genes, and the same bytes
    under no_fuse, no_duo, solver_no_wave and no_seg."""
    prm = pa.make_params(**KP)
    lone = [pa.synth_contig(5100, 60000).decode()]
    rng = np.random.RandomState(61)
    small = [[pa.synth_contig(6100 + 10 * n + i, int(rng.choice([600, 3000, 6000, 9000]))).decode() for i in range(n)] for n in (1, 2, 3, 4)]
    medium = fuzz(62, 40)
    batches = [lone] + small + [medium]
    want = {}
    for b, seqs in enumerate(batches):
        ann = pa.Annotator(prm)
        st, offs, genes = run3(ann, seqs)
        o = list(pool.map(orc, [(s, KP) for s in seqs], chunksize=2))
        compare(ann, seqs, KP, st, offs, genes, o)
        if b == 0:
            assert ann.seg_runs() >= 1 and st[0] == 0 and offs[1] > 0
        elif b <= 4:
            assert ann.front_runs() == 2, (b, ann.front_runs())
        want[b] = (st.tobytes(), offs.tobytes(), genes.tobytes())
        ann.close()
    for fl in ("no_fuse", "no_duo", "solver_no_wave", "no_seg"):
        for b, seqs in enumerate(batches):
            ann = pa.Annotator(pa.make_params(**KP), flags=(fl,))
            st, offs, genes = run3(ann, seqs)
            assert (st.tobytes(), offs.tobytes(), genes.tobytes()) == want[b], (fl, b)
            if fl == "no_fuse" and 1 <= b <= 4:
                assert ann.front_runs() == 0
            if fl == "no_seg":
                assert ann.seg_runs() == 0
            ann.close()
    seqs = fuzz(63, 720)
    ann = pa.Annotator(pa.make_params(**KP))
    ann.upload(seqs)
    ann.run()
    st, offs, genes = ann.download_flat()
    o = list(pool.map(orc, [(s, KP) for s in seqs], chunksize=8))
    n, by_dec, beyond, same = compare(ann, seqs, KP, st, offs, genes, o)
    assert n >= 700 and len(same) >= 500, (n, by_dec, beyond, len(same))
    ann.close()


def test_drawn_flags_fuzz(pa, oracle, pool):
    """tools/fuzz_params.py bounded: 10 flag sets drawn with a fixed seed (overlapping classes, repeated codons, up to 16 starts, upper
    case, exponent / zero / negative weights, minlen around the multiples of 3), 40 contigs each.  The fuzz rule against the oracle; on
    two small contigs per batch the certificate's statement: k_refine's bounds hold the reference's integers (Python's decimal, raw
    flags) and the contig is certified or solved again."""
    import certify_probe
    import decimal_replay as dump
    import fuzz_params

    rng = np.random.RandomState(2026)
    tot = n_bounds = 0
    for b in range(10):
        kw = fuzz_params.draw_flags(rng)
        seqs = fuzz(900 + b, 40)
        ann = pa.Annotator(pa.make_params(**kw))
        ann.upload(seqs)
        ann.run()
        st, offs, genes = ann.download_flat()
        want = list(pool.map(orc, [(s, kw) for s in seqs], chunksize=2))
        n, by_dec, beyond, same = compare(ann, seqs, kw, st, offs, genes, want)
        tot += n
        cert = ann.certified()
        small = [i for i in range(len(seqs)) if st[i] == 0 and len(seqs[i]) <= 6000 and ann.globals(i).n_edge > 0]
        for i in small[:2]:
            assert cert[i] in (1, 2), (b, i, kw)
            viol = certify_probe.bounds_hold(ann.edges(i), dump.decimal_weights(ann, i, seqs[i], kw["start_codons"])[2])
            assert not viol, (b, i, kw, viol[:3])
            n_bounds += 1
        ann.close()
    assert tot >= 380 and n_bounds >= 10, (tot, n_bounds)


def test_exactness_on_the_fixture_flags(pa):
    """The certificate's statement on a fixture contig and on 3 small fuzz contigs per raw flag set of the fixtures."""
    import certify_probe
    import decimal_replay as dump

    n_edges = n_flag = 0
    for k, case in enumerate(PARAM_CASES):
        g, name, seq = load_golden(case)
        kw = raw_flags(g)
        seqs = [seq] + [s for s in fuzz(1000 + k, 12) if len(s) <= 6000][:3]
        ann = pa.Annotator(pa.make_params(**kw))
        ann.upload(seqs)
        ann.run()
        st, offs, genes = ann.download_flat()
        cert = ann.certified()
        for i in range(len(seqs)):
            if st[i] != 0 or ann.globals(i).n_edge == 0:
                continue
            assert cert[i] in (1, 2), (case, i)
            ed = ann.edges(i)
            viol = certify_probe.bounds_hold(ed, dump.decimal_weights(ann, i, seqs[i], kw["start_codons"])[2])
            assert not viol, (case, i, viol[:3])
            n_edges += len(ed)
            n_flag += int(ed["inexact"].sum())
        ann.close()
    assert n_edges > 50000 and n_flag > 0, (n_edges, n_flag)


@pytest.mark.parametrize("case", ["param_start_rc_stop", "param_16_starts", "param_minlen7", "param_repeated"])
def test_margins_and_drops(case, pa):
    import test_drop_gpu
    import test_margins_gpu

    g, name, seq = load_golden(case)
    kw = raw_flags(g)
    seqs = [seq] + [s for s in fuzz(1100 + PARAM_CASES.index(case), 16) if len(s) <= 12000]
    ann = pa.Annotator(pa.make_params(**kw))
    mst, _, rec = test_margins_gpu.run_and_check(ann, seqs)
    assert mst[0] == 0 and len(rec) > 0
    dst, _, drec = test_drop_gpu.run_and_check(ann, seqs, sample=6, seed=PARAM_CASES.index(case))
    assert dst[0] == 0
    ann.close()


def test_cli_prints_the_fixture_tabular(tmp_path):
    """phanotate.py -s RAW -e RAW -l N fixture.fasta.gz: exactly the reference's tabular text."""
    for case in PARAM_CASES:
        g, name, seq = load_golden(case)
        kw = raw_flags(g)
        args = [sys.executable, os.path.join(ROOT, "phanotate.py"), "-s", kw["start_codons"], "-e", kw["stop_codons"], "-l", str(kw["minlen"]),
                os.path.join(GOLDEN, case + ".fasta.gz")]
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (case, r.stderr[-2000:])
        assert r.stdout == str(g["tabular"]), case
