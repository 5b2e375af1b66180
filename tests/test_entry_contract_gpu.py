"""The call-sequence contract of the entry points that read a finished run, through ctypes: PHX_E_STATE (-13) before any run and after a
new upload, a run in flight settled by the entry itself, PHX_E_ARG (-1) for missing output arrays, and the size query / short cap /
exact cap protocol of the flat calls.  One batch with a contig that fails (status < 0) between two that do not."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -13


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Calls:
    """The nine entries on one context.  Each method makes the call in one of three forms — "query": every output array but the records
    (the size query), "null": the output arrays missing, a number: records with that capacity — and returns (rc, total reported)."""

    def __init__(self, ann, n):
        from phanotate_amd import _lib

        self.L, self.h, self.n, self.lib = ann.L, ann.h, n, _lib
        self.offs = np.zeros(n + 1, np.int64)
        self.status = np.zeros(n, np.int32)
        self.delta = np.zeros(n, np.float64)
        self.oo = np.zeros(n + 1, np.int64)  # filled by orf_offsets("query") once a run has finished
        self.repl_k = 0                     # tap_replacement: the record of contig 0 asked for

    def _flat(self, fn, dt, form):
        total = C.c_int64(-7)
        if form == "null":
            return fn(self.h, None, 0, None, None, C.byref(total)), total.value
        rec = None if form == "query" else np.empty(max(form, 1), dt)
        rc = fn(self.h, None if rec is None else vp(rec), 0 if rec is None else form, vp(self.offs), vp(self.status), C.byref(total))
        return rc, total.value

    def download_flat(self, form):
        return self._flat(self.L.phx_download_flat, self.lib.GENE_DT, form)

    def margins_flat(self, form):
        return self._flat(self.L.phx_margins_flat, self.lib.MARGIN_DT, form)

    def drop_margins_flat(self, form):
        return self._flat(self.L.phx_drop_margins_flat, self.lib.DROP_DT, form)

    def certified(self, form):
        cert = np.zeros(self.n, np.int8)
        return self.L.phx_certified(self.h, None if form == "null" else vp(cert)), None

    def replacements_flat(self, form):
        total, gtotal = C.c_int64(-7), C.c_int64(-7)
        if form == "null":
            return self.L.phx_replacements_flat(self.h, None, 0, None, 0, None, None, C.byref(total), C.byref(gtotal)), total.value
        if form == "query":
            return self.L.phx_replacements_flat(self.h, None, 0, None, 0, vp(self.offs), vp(self.status), C.byref(total), C.byref(gtotal)), total.value
        rec = np.empty(max(form, 1), self.lib.REPL_DT)
        genes = np.empty(1 << 16, self.lib.GENE_DT)
        rc = self.L.phx_replacements_flat(self.h, vp(rec), form, vp(genes), len(genes), vp(self.offs), vp(self.status), C.byref(total), C.byref(gtotal))
        assert 0 <= gtotal.value <= len(genes)
        return rc, total.value

    def tap_replacement(self, form):
        n = C.c_int32(-7)
        if form == "null":
            return self.L.phx_tap_replacement(self.h, 0, self.repl_k, None, 0, None), None
        path = None if form == "query" else np.empty(max(form, 1), np.int32)
        return self.L.phx_tap_replacement(self.h, 0, self.repl_k, None if path is None else vp(path), 0 if path is None else form, C.byref(n)), n.value

    def orf_offsets(self, form):
        return self.L.phx_orf_offsets(self.h, None if form == "null" else vp(self.oo)), None

    def reannotate_flat(self, form):
        total = C.c_int64(-7)
        mask = np.zeros(max(int(self.oo[self.n]), 1), np.uint8)
        if form == "null":
            return self.L.phx_reannotate_flat(self.h, vp(mask), vp(self.oo), 1, None, 0, None, None, None, C.byref(total)), total.value
        genes = None if form == "query" else np.empty(max(form, 1), self.lib.GENE_DT)
        rc = self.L.phx_reannotate_flat(self.h, vp(mask), vp(self.oo), 1, None if genes is None else vp(genes), 0 if genes is None else form,
                                        vp(self.offs), vp(self.status), vp(self.delta), C.byref(total))
        return rc, total.value

    def tap_path(self, form):
        n = C.c_int32(-7)
        if form == "null":  # (no output array is required: the argument this tap refuses is the contig)
            return self.L.phx_tap_path(self.h, self.n, None, 0, C.byref(n), None, 0), None
        path = None if form == "query" else np.empty(max(form, 1), np.int32)
        return self.L.phx_tap_path(self.h, 0, None if path is None else vp(path), 0 if path is None else form, C.byref(n), None, 0), n.value


ENTRIES = ["download_flat", "certified", "margins_flat", "drop_margins_flat", "replacements_flat", "tap_replacement", "orf_offsets", "reannotate_flat", "tap_path"]
SIZED = ["download_flat", "margins_flat", "drop_margins_flat", "replacements_flat", "tap_replacement", "reannotate_flat", "tap_path"]


def test_entry_contract():
    import phanotate_amd as pa

    seqs = [pa.synth_contig(41, 6000), b"acg", pa.synth_contig(42, 9000)]
    ann = pa.Annotator(device=0)
    try:
        ann.upload(seqs)
        k = Calls(ann, len(seqs))
        for name in ENTRIES:  # a batch, no run yet
            assert getattr(k, name)("query")[0] == E_STATE, name
        ann.run()  # (a context's first run is synchronous)
        assert k.orf_offsets("query")[0] == 0 and k.oo[len(seqs)] > 0
        for name in ENTRIES:  # the entry itself settles a run in flight
            ann.run_async()
            assert getattr(k, name)("query")[0] == 0, name
        assert k.status[1] < 0 and k.status[0] >= 0 and k.status[2] >= 0
        for name in ENTRIES:
            assert getattr(k, name)("null")[0] == E_ARG, name
        # a record of contig 0 whose replacement has a path to report
        rc, ndrop = k.drop_margins_flat("query")
        assert rc == 0 and k.offs[1] - k.offs[0] > 0
        for r in range(int(k.offs[1] - k.offs[0])):
            k.repl_k = r
            rc, total = k.tap_replacement("query")
            assert rc == 0
            if total > 0:
                break
        for name in SIZED:
            call = getattr(k, name)
            rc, total = call("query")
            assert rc == 0 and total > 0, name
            assert call(total - 1) == (E_ARG, total), name  # one short: refused, the total still reported
            assert call(total) == (0, total), name
        ann.upload(seqs)
        for name in ENTRIES:
            assert getattr(k, name)("query")[0] == E_STATE, name
    finally:
        ann.close()
