"""Host-side front end of libphx: parameter handling, batching, result unpacking.

Mirrors the way phanotate.py drives the path (phanotate.py:40-76): per contig
get_orfs -> get_graph -> shortest path -> features; here a whole batch of contigs goes
through the HIP kernels at once.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import PhxError


def make_params(start_codons="atg:0.85,gtg:0.10,ttg:0.05", stop_codons="tag,tga,taa", minlen=90):
    """Same flag syntax and normalisation as file_handling.get_args (file_handling.py:51-66): phx_params_from_flags.  The weights also
    travel as the texts the user wrote (phx_params.start_w_text): the reference holds Decimal(text) / max."""
    p = _lib.Params()
    rc = _lib.lib().phx_params_from_flags(start_codons.encode(), stop_codons.encode(), int(minlen), C.byref(p))
    if rc:
        raise ValueError("start / stop codons %r / %r, minlen %r: libphx takes codon:weight pairs and codons of exactly 3 letters out of acgt, "
                         "at most %d of each, minlen >= 6 (%s)" % (start_codons, stop_codons, minlen, _lib.MAXC, _lib.lib().phx_strerror(rc).decode()))
    p.start_codons_text = start_codons  # the flag as given (dump.py's Decimal replay reads it)
    return p


def synth_contig(seed, L=50000):
    """Deterministic synthetic phage-like contig (host utility of libphx)."""
    buf = C.create_string_buffer(int(L))
    rc = _lib.lib().phx_synth_contig(int(seed), int(L), buf)
    if rc:
        raise PhxError(rc, "phx_synth_contig")
    return buf.raw


def _limbs_to_int(limbs, nl):
    """The signed python int of nl 64-bit limbs, least significant first (two's complement across the limbs)."""
    v = 0
    for k in range(nl):
        v |= int(limbs[k]) << (64 * k)
    return v - (1 << (64 * nl)) if v >> (64 * nl - 1) else v


def _dist_list(rows, nl):
    """Per-node distances of a limb array (one row of w words per node) of a contig of nl limbs as python ints; None: unreached (a value
    at or above 2^(64 w - 3)).  w == nl + 1 is a vector of a contig solved with required ORFs: x = S - count * 2^(64 nl), |S| < 2^(64 nl) / 2,
    comes out as (S, count)."""
    out = []
    for row in rows:
        w = len(row)
        x = _limbs_to_int(row, w)
        if x >= 1 << (64 * w - 3):
            out.append(None)
        elif w <= nl:
            out.append(x)
        else:
            M = 1 << (64 * nl)
            count = (-x + M // 2) // M
            out.append((x + count * M, count))
    return out


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# the *_ms getters: library call -> the names of its spans
_MS_KEYS = {
    "phx_margins_ms": ("transpose", "reverse", "margins", "download"),
    "phx_drop_ms": ("trees", "candidates", "fixups", "download"),
    "phx_replacements_ms": ("argmin", "walk", "download"),
    "phx_profile_ms": ("tables", "records", "download"),
    "phx_scenarios_ms": ("mask", "solve", "finish"),
    "phx_remargins_ms": ("apply", "reverse", "margins", "download"),
    "phx_pinmargins_ms": ("apply", "reverse", "margins", "download"),
    "phx_redrops_ms": ("trees", "candidates", "fixups", "download"),
    "phx_reprofile_ms": ("tables", "records", "download"),
    "phx_pinprofile_ms": ("tables", "records", "download"),
    "phx_pindrops_ms": ("trees", "candidates", "fixups", "download"),
    "phx_rereplacements_ms": ("argmin", "walk", "download"),
    "phx_pinreplacements_ms": ("argmin", "walk", "download"),
    "phx_reannotate_ms": ("mask", "solve", "finish"),
}


class Pool:
    """phx_pool: ONE call annotates a list of contigs over several GPUs from this process — a host thread and two contexts per device
    inside the library, batches round the devices, results in input order.  devices: GPU ordinals (one may repeat)."""

    def __init__(self, params=None, devices=(0,), flags=()):
        self.L = _lib.lib()
        self.params = params or make_params()
        fl = 0
        for f in flags:
            fl |= Annotator.FLAGS[f]
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.L.phx_pool_create(C.byref(self.params), len(devices), devs, fl, C.byref(h))
        if rc:
            raise PhxError(rc, "%s (%s)" % (self.L.phx_strerror(rc).decode(), self.L.phx_last_error(None).decode()))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.phx_pool_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def annotate(self, seqs, trnas=None, batch_bases=0):
        """[(status, genes structured array)] per contig, in input order (phx_pool_annotate)."""
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(seqs)
        arr = (C.c_char_p * max(n, 1))(*seqs)
        lens = (C.c_int64 * max(n, 1))(*[len(s) for s in seqs])
        res = (_lib.Result * max(n, 1))()
        to = ta = tz = None
        if trnas is not None:
            offs = np.zeros(n + 1, np.int64)
            np.cumsum([len(t) for t in trnas], out=offs[1:])
            a = np.ascontiguousarray([h[0] for t in trnas for h in t] or [0], np.int32)
            z = np.ascontiguousarray([h[1] for t in trnas for h in t] or [0], np.int32)
            to, ta, tz = (x.ctypes.data_as(C.c_void_p) for x in (offs, a, z))
        rc = self.L.phx_pool_annotate(self.h, n, arr, lens, int(batch_bases), to, ta, tz, res)
        if rc:
            raise PhxError(rc, "phx_pool_annotate: %s (%s)" % (self.L.phx_strerror(rc).decode(), self.L.phx_pool_last_error(self.h).decode()))
        out = []
        for i in range(n):
            g = np.zeros(res[i].n_genes, _lib.GENE_DT)
            if res[i].n_genes:
                C.memmove(g.ctypes.data, res[i].genes, res[i].n_genes * _lib.GENE_DT.itemsize)
            out.append((int(res[i].status), g))
        self.L.phx_free_results(res, n)
        return out


class Annotator:
    """One libphx context = one (host thread, GPU).

    `stream`: None lets the context create its own (non-blocking) stream; an int is a raw hipStream_t used as given —
    0 is HIP's null stream, which is what `torch.cuda.current_stream().cuda_stream` returns by default, so that the
    context's work is ordered after the caller's on that stream (phx_create_ex, PHX_CREATE_USE_STREAM)."""

    FLAGS = {"no_graph": 2, "size_every_run": 4, "solver_global": 8, "solver_no_wave": 16, "no_certify": 32, "cert_tight": 64, "cert_wide": 128, "poison": 256, "one_stream": 512, "no_exact": 1024, "no_fuse": 2048, "no_duo": 4096, "no_seg": 8192, "no_chain": 16384}  # PHX_CREATE_* development / test switches

    def __init__(self, params=None, device=0, stream=None, flags=()):
        self.L = _lib.lib()
        self.params = params or make_params()
        h = C.c_void_p()
        fl = 0
        for f in flags:
            fl |= self.FLAGS[f]
        if stream is None:
            rc = self.L.phx_create_ex(C.byref(self.params), int(device), None, fl, C.byref(h))
        else:
            rc = self.L.phx_create_ex(C.byref(self.params), int(device), C.c_void_p(int(stream)), 1 | fl, C.byref(h))
        if rc:
            raise PhxError(rc, "%s (%s)" % (self.L.phx_strerror(rc).decode(), self.L.phx_last_error(None).decode()))
        self.h = h
        self.n = 0

    def close(self):
        if getattr(self, "h", None):
            self.L.phx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            raise PhxError(rc, "%s: %s (%s)" % (what, self.L.phx_strerror(rc).decode(), self.L.phx_last_error(self.h).decode()))

    def _ms(self, name):
        keys = _MS_KEYS[name]
        ms = (C.c_float * len(keys))()
        self._chk(getattr(self.L, name)(self.h, ms), name)
        return dict(zip(keys, [float(x) for x in ms]))

    def _query_fill(self, fn, name, head, count, dts, layout="rc", per=(np.int32,)):
        """The size query and the fill of one *_flat entry point: fn(handle, *head, <records>, offsets, *per-entry arrays, *totals).
        `layout` spells the records' arguments — r: the next array of `dts`, c: the capacity of the arrays since the last c, which the
        next total sizes (null and 0 in the size query).  `per`: dtypes of the arrays with one value per entry (status first), `count`
        entries.  Returns (per-entry arrays cut to count, offsets, record arrays cut to their totals)."""
        offs = np.zeros(count + 1, np.int64)
        ent = [np.zeros(max(count, 1), dt) for dt in per]
        totals = [C.c_int64(0) for _ in range(layout.count("c"))]
        sized_by = [layout[:k].count("c") for k, ch in enumerate(layout) if ch == "r"]
        recs = [None] * len(dts)
        for fill in (False, True):
            if fill:
                recs = [np.empty(max(int(totals[t].value), 1), dt) for t, dt in zip(sized_by, dts)]
            it = iter(recs)
            block = []
            for ch in layout:
                if ch == "r":
                    a = next(it)
                    block.append(_vp(a) if fill else None)
                else:
                    block.append(len(a) if fill else 0)
            self._chk(fn(self.h, *head, *block, _vp(offs), *[_vp(a) for a in ent], *[C.byref(t) for t in totals]), name)
        return [a[:count] for a in ent], offs, [a[: int(totals[t].value)] for t, a in zip(sized_by, recs)]

    def _tap_path(self, fn, name, g, *ids):
        """(path as device node ids, its length as a python int) from one of the path taps of a contig with globals g."""
        p = np.zeros(max(g.n_node, 1), np.int32)
        n = C.c_int32()
        limbs = np.zeros(32, np.uint64)
        self._chk(fn(self.h, *ids, _vp(p), len(p), C.byref(n), _vp(limbs), 32), name)
        return p[: n.value].copy(), _limbs_to_int(limbs, max(g.n_limbs, 1))

    def _tap_dist(self, fn, name, i, *which, pinned=False):
        """_dist_list of one of the distance taps of contig i; pinned: the tap may deliver one word more per node and says how many."""
        g = self.globals(i)
        nl, V = max(g.n_limbs, 1), max(g.n_node, 0)
        a = np.zeros((max(V, 1), nl + (1 if pinned else 0)), np.uint64)
        wpn = C.c_int32(0)
        self._chk(fn(self.h, i, *which, _vp(a), a.size, *((C.byref(wpn),) if pinned else ())), name)
        w = min(int(wpn.value) or nl, nl + 1) if pinned else nl
        return _dist_list(a.reshape(-1)[: V * w].reshape(V, w), nl)

    def _device_lists(self):
        """download_flat(exact=False)'s arrays: the device's own lists for every contig."""
        self._chk(self.L.phx_set_exact(self.h, 0), "phx_set_exact")
        try:
            return self._download_flat()
        finally:
            self._chk(self.L.phx_set_exact(self.h, 1), "phx_set_exact")

    def _gene_changes(self, contigs, roffs, rgenes, soffs, genes):
        """For every scenario x of contig contigs[x] whose new annotation is genes[soffs[x]:soffs[x+1]], against the run's device lists
        (roffs, rgenes of _device_lists): (keys of the run's genes, keys of the new ones, orfs(contig), n_removed, n_added), a key being
        (left, right, strand, frame)."""
        key = lambda g: (int(g["left"]), int(g["right"]), int(g["strand"]), int(g["frame"]))
        have, have_of, orfs_of = None, -1, None
        for x, i in enumerate(contigs):
            if have_of != i:
                have, have_of, orfs_of = {key(g) for g in rgenes[roffs[i]:roffs[i + 1]]}, i, self.orfs(i)
            new = {key(g) for g in genes[soffs[x]:soffs[x + 1]]}
            yield have, new, orfs_of, len(have - new), len(new - have)

    # ---- the path ----
    def upload(self, seqs):
        seqs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(seqs)
        arr = (C.c_char_p * n)(*seqs)
        lens = (C.c_int64 * n)(*[len(s) for s in seqs])
        self._keep = (seqs, arr, lens)
        self._chk(self.L.phx_upload(self.h, n, arr, lens), "phx_upload")
        self.n = n
        self._orf_offs = None

    def upload_raw(self, ptrs, lens, keep=None):
        """The same from raw addresses: ptrs uint64[n] (host memory that stays valid for the call), lens int64[n]."""
        ptrs = np.ascontiguousarray(ptrs, np.uint64)
        lens = np.ascontiguousarray(lens, np.int64)
        self._keep = (ptrs, lens, keep)
        self._chk(self.L.phx_upload(self.h, len(lens), C.cast(ptrs.ctypes.data, C.POINTER(C.c_char_p)), C.cast(lens.ctypes.data, C.POINTER(C.c_int64))), "phx_upload")
        self.n = len(lens)
        self._orf_offs = None

    def attach(self, dev_ptr, offsets):
        """Concatenated ASCII already in HBM (e.g. a torch uint8 tensor's data_ptr()); offsets has n+1 entries."""
        offs = (C.c_int64 * len(offsets))(*[int(x) for x in offsets])
        self._keep = (offs,)
        self._chk(self.L.phx_attach(self.h, len(offsets) - 1, C.c_void_p(int(dev_ptr)), offs), "phx_attach")
        self.n = len(offsets) - 1
        self._orf_offs = None

    def set_trnas(self, trnas):
        """tRNA hits for the batch just uploaded: one list of (start, stop) per contig, as functions.add_trnas holds them
        (start > stop for a complement hit); None = no tRNA finder installed (functions.py:493-495)."""
        if trnas is None:
            self._chk(self.L.phx_set_trnas(self.h, None, None, None), "phx_set_trnas")
            return
        if len(trnas) != self.n:
            raise ValueError("one hit list per contig of the batch")
        offs = np.zeros(self.n + 1, np.int64)
        np.cumsum([len(t) for t in trnas], out=offs[1:])
        a = np.ascontiguousarray([h[0] for t in trnas for h in t] or [0], np.int32)
        z = np.ascontiguousarray([h[1] for t in trnas for h in t] or [0], np.int32)
        vp = lambda x: x.ctypes.data_as(C.c_void_p)
        self._chk(self.L.phx_set_trnas(self.h, vp(offs), vp(a), vp(z)), "phx_set_trnas")

    def run(self):
        self._chk(self.L.phx_run(self.h), "phx_run")
        self._orf_offs = None

    def run_async(self):
        """Enqueue the run and return (phx_run_async); wait() — or any other call on this context — collects it.  With two
        contexts alternating, one batch's upload and kernels overlap the other's shortest-path kernel: see pipeline.Pipeline."""
        self._chk(self.L.phx_run_async(self.h), "phx_run_async")
        self._orf_offs = None

    def wait(self):
        self._chk(self.L.phx_wait(self.h), "phx_wait")

    def set_exact(self, on):
        """phx_set_exact: off — the downloads hand out the device's own lists (no certificate, no host re-solve) and run_async does not
        put the certificate kernels behind the run."""
        self._chk(self.L.phx_set_exact(self.h, 1 if on else 0), "phx_set_exact")

    def download_flat(self, exact=True):
        """(status int32[n], offsets int64[n+1], genes structured array[total]): genes of contig i are genes[offsets[i]:offsets[i+1]]
        in path order (phx_download_flat: no per-contig allocation).  The library delivers the reference's genes: a contig the device
        could not certify against the reference's Decimal-derived integers (phx_certified; none is expected) is solved again on those
        integers inside phx_download_flat (csrc/phx_exact.inc); its indices are then in self.resolved.  exact=False: the device's
        own lists for every contig (phx_set_exact; tests and measurements)."""
        if not exact:
            res = self._device_lists()
            self.resolved = []
            return res
        res = self._download_flat()
        self.resolved = [int(i) for i in np.nonzero(self.certified() == 2)[0]] if self.n else []
        return res

    def _download_flat(self):
        n = self.n
        offs = np.zeros(n + 1, np.int64)
        status = np.zeros(max(n, 1), np.int32)
        total = C.c_int64(0)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        # one call when the gene array of the size the last batch needed (plus a margin) is large enough: phx_download_flat reports the
        # total and copies nothing if it is not
        guess = max(int(getattr(self, "_genes_seen", 0) * 1.25) + 64, 1)
        genes = np.empty(guess, _lib.GENE_DT)
        rc = self.L.phx_download_flat(self.h, vp(genes), len(genes), vp(offs), vp(status), C.byref(total))
        if rc == -1 and int(total.value) > len(genes):  # too small: the total is known now
            genes = np.empty(int(total.value), _lib.GENE_DT)
            rc = self.L.phx_download_flat(self.h, vp(genes), len(genes), vp(offs), vp(status), C.byref(total))
        self._chk(rc, "phx_download_flat")
        self._genes_seen = int(total.value)
        return status[:n], offs, genes[: int(total.value)]

    def certified(self):
        """int8[n]: 1 the contig's genes are proven on the device to be what the reference's Decimal-derived integers give
        (phx_certified), 2 not proven there and solved again on those integers on the host (inside the library), 0 neither,
        -1 the context runs without the certificate."""
        c = np.zeros(max(self.n, 1), np.int8)
        self._chk(self.L.phx_certified(self.h, c.ctypes.data_as(C.c_void_p)), "phx_certified")
        return c[: self.n]

    def download(self):
        """[(status, genes structured array)] per contig; the arrays are views into one flat buffer (phx_download_flat)."""
        status, offs, genes = self.download_flat()
        o = offs.tolist()
        st = status.tolist()
        return [(st[i], genes[o[i]:o[i + 1]]) for i in range(self.n)]

    def annotate(self, seqs, trnas=None):
        """[(status, genes structured array)] for every contig, in input order.  trnas: see set_trnas."""
        self.upload(seqs)
        if trnas is not None:
            self.set_trnas(trnas)
        self.run_async()  # (the certificate the download asks for goes behind the run on the stream; the download waits for both)
        return self.download()

    def annotate_flat(self, seqs):
        """The same as three flat arrays, see download_flat."""
        self.upload(seqs)
        self.run_async()
        return self.download_flat()

    def annotate_flat_raw(self, ptrs, lens, keep=None):
        """annotate_flat for a caller that holds the C-ABI's own arguments: the contigs' addresses (uint64[n]) and lengths (int64[n])."""
        self.upload_raw(ptrs, lens, keep)
        self.run_async()
        return self.download_flat()

    def dump_text(self, i):
        """-d/--dump of the reference for contig i of the batch last run (phx_dump_text): bytes, one line per edge."""
        text, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.phx_dump_text(self.h, int(i), C.byref(text), C.byref(n)), "phx_dump_text")
        out = C.string_at(text.value, n.value)
        self.L.phx_free_text(text)
        return out

    # ---- stage taps (parity tests) ----
    def globals(self, i):
        g = _lib.Globals()
        self._chk(self.L.phx_tap_globals(self.h, i, C.byref(g)), "phx_tap_globals")
        return g

    def positions(self, i):
        L = int(self.globals(i).L)
        a = [np.zeros(L, np.uint8) for _ in range(4)]
        self._chk(self.L.phx_tap_positions(self.h, i, *[x.ctypes.data_as(C.c_void_p) for x in a]), "phx_tap_positions")
        return dict(cls=a[0], gcc=a[1], binF=a[2], binR=a[3])

    def orfs(self, i):
        g = self.globals(i)
        a = np.zeros(max(g.n_orf, 0), _lib.ORF_DT)
        self._chk(self.L.phx_tap_orfs(self.h, i, a.ctypes.data_as(C.c_void_p)), "phx_tap_orfs")
        return a

    def nodes(self, i):
        g = self.globals(i)
        a = np.zeros(max(g.n_node, 0), _lib.NODE_DT)
        self._chk(self.L.phx_tap_nodes(self.h, i, a.ctypes.data_as(C.c_void_p)), "phx_tap_nodes")
        return a

    def edges(self, i):
        g = self.globals(i)
        a = np.zeros(max(g.n_edge, 0), _lib.EDGE_DT)
        self._chk(self.L.phx_tap_edges(self.h, i, a.ctypes.data_as(C.c_void_p)), "phx_tap_edges")
        return a

    def path(self, i):
        return self._tap_path(self.L.phx_tap_path, "phx_tap_path", self.globals(i), i)

    def dist(self, i):
        """Exact distance of every node from the source as python ints (None: unreached), device node order."""
        return self._tap_dist(self.L.phx_tap_dist, "phx_tap_dist", i)

    def dist_to_target(self, i):
        """Exact distance of every node TO the target as python ints (None: no path to the target), device node order
        (phx_tap_dist_target; the margins' reverse pass, computed on the first call after a run)."""
        return self._tap_dist(self.L.phx_tap_dist_target, "phx_tap_dist_target", i)

    def margins(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.MARGIN_DT): the path margin of every CDS ORF of
        the batch last run (phx_margins_flat).  The records of contig i are records[offsets[i]:offsets[i+1]], in the order of orfs(i);
        margin = float(d_s(u) + W + d_t(v) - D) / 1000 (0 for a called ORF of a certified contig, +inf where no path runs through the ORF);
        status as phx_margins_flat reports it (< 0: no records)."""
        (status,), offs, (rec,) = self._query_fill(self.L.phx_margins_flat, "phx_margins_flat", (), self.n, (_lib.MARGIN_DT,))
        return status, offs, rec

    def margins_ms(self):
        """Device time of the last margins computation in ms: out-edge CSR, reverse pass, records, copy to the host (phx_margins_ms)."""
        return self._ms("phx_margins_ms")

    def drop_margins(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.DROP_DT): the drop margin of every CDS gene of
        the device path of every contig of the batch last run (phx_drop_margins_flat), in path order.  drop = float(D_{-g} - D) / 1000,
        D_{-g} the shortest source -> target distance without the gene's stop node (+inf with bypass = 0 where no path avoids it);
        called = 1 for the genes download_flat() delivers; status as phx_drop_margins_flat reports it (!= 0: no records)."""
        (status,), offs, (rec,) = self._query_fill(self.L.phx_drop_margins_flat, "phx_drop_margins_flat", (), self.n, (_lib.DROP_DT,))
        return status, offs, rec

    def drop_ms(self):
        """Device time of the last drop-margins computation in ms: trees + labels, candidates, fixups, copy to the host (phx_drop_ms)."""
        return self._ms("phx_drop_ms")

    def profile(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.PROFILE_DT): the coding profile of every contig of
        the batch last run (phx_profile_flat).  The n_node - 1 records of contig i are records[offsets[i]:offsets[i+1]], one
        per slot between neighbouring nodes of nodes(i) (lo, hi: their pos; 0 and L + 1 at the ends).  fwd / rev / gap: the smallest path
        margin float(d_s(u) + W + d_t(v) - D) / 1000 over the forward gene edges / reverse gene edges / connectors that cover the slot, +inf
        where none does — what it costs the best annotation to have the stretch inside a forward gene, inside a reverse gene, between genes.
        status as phx_profile_flat reports it (< 0: no records; 1: no path, every value +inf)."""
        (status,), offs, (rec,) = self._query_fill(self.L.phx_profile_flat, "phx_profile_flat", (), self.n, (_lib.PROFILE_DT,))
        return status, offs, rec

    def profile_ms(self):
        """Device time of the last profile computation in ms: candidates + tables + push-down, the slots' bounds, copy to the host (phx_profile_ms)."""
        return self._ms("phx_profile_ms")

    def replacements(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.REPL_DT, genes structured array of _lib.GENE_DT):
        for every record of drop_margins() (same order, statuses and offsets; drop, called and bypass bit-equal) what the best path
        without the gene calls instead (phx_replacements_flat).  Record r's genes are genes[r.gene_off:][:r.n_removed]
        (the device path's genes the replacement drops, the gene itself among them), then the next r.n_added (the genes it calls
        instead), in path order."""
        (status,), offs, (rec, genes) = self._query_fill(self.L.phx_replacements_flat, "phx_replacements_flat", (), self.n, (_lib.REPL_DT, _lib.GENE_DT), "rcrc")
        return status, offs, rec, genes

    def replacement_path(self, i, k):
        """R_g of record k of contig i (replacements()[2][offsets[i] + k]): device node ids, source first; empty when bypass = 0."""
        n = C.c_int32()
        self._chk(self.L.phx_tap_replacement(self.h, i, k, None, 0, C.byref(n)), "phx_tap_replacement")
        p = np.zeros(max(n.value, 1), np.int32)
        self._chk(self.L.phx_tap_replacement(self.h, i, k, p.ctypes.data_as(C.c_void_p), len(p), C.byref(n)), "phx_tap_replacement")
        return p[: n.value].copy()

    def replacements_ms(self):
        """Device time of the last replacements computation in ms: argmin, walk + genes, copy to the host (phx_replacements_ms)."""
        return self._ms("phx_replacements_ms")

    def replacement_stats(self):
        """Counters of the last replacements computation (phx_replacement_stats): slots won by a cross candidate, their delta-chain nodes,
        cross winners whose path keeps its delta chain, walks whose zero-length loop was cut, 1 when the delta-chain buffer had to grow."""
        out = (C.c_int64 * 5)()
        self._chk(self.L.phx_replacement_stats(self.h, out), "phx_replacement_stats")
        return dict(zip(("cross", "chain_nodes", "cross_kept", "cut", "regrown"), [int(x) for x in out]))

    # ---- masked re-annotation ----
    def orf_offsets(self):
        """int64[n+1]: cumulative ORF counts of the batch last run, the offsets margins() reports (a contig with a run error or without
        device distances counts no ORFs; phx_orf_offsets)."""
        if getattr(self, "_orf_offs", None) is None:
            offs = np.zeros(self.n + 1, np.int64)
            self._chk(self.L.phx_orf_offsets(self.h, offs.ctypes.data_as(C.c_void_p)), "phx_orf_offsets")
            self._orf_offs = offs
        return self._orf_offs

    def orf_index(self, i, left, right, strand):
        """Index in orfs(i) of the ORF with these ends (left, right and strand as a gene record carries them: right includes the stop
        codon).  KeyError when contig i has no such ORF."""
        cache = getattr(self, "_orf_index", None)
        if cache is None or cache[0] is not self.orf_offsets() or cache[1] != i:
            o = self.orfs(i)
            fwd = o["frame"] > 0
            lo = np.where(fwd, o["start"], o["stop"])
            hi = np.where(fwd, o["stop"], o["start"]) + 2
            table = {}
            for k, key in enumerate(zip(lo.tolist(), hi.tolist(), fwd.tolist())):
                table.setdefault(key, k)
            cache = self._orf_index = (self.orf_offsets(), i, table)
        try:
            return cache[2][(int(left), int(right), int(strand) > 0)]
        except KeyError:
            raise KeyError("contig %d has no ORF %d..%d on strand %+d" % (i, left, right, 1 if int(strand) > 0 else -1)) from None

    def reannotate(self, forbid, solve_all=False):
        """(status int32[n], offsets int64[n+1], genes structured array[total], delta float64[n]): the batch last run annotated again
        without the ORFs of `forbid` — one array of indices into orfs(i) per contig, or None — on the resident device graph
        (phx_reannotate_flat).  genes[offsets[i]:offsets[i+1]] are contig i's, in the format and order of download_flat(exact=False);
        delta[i] = float(D_F - D) / 1000 (+inf: no path without them, status 1).  A contig with an empty mask keeps the run's result
        unless solve_all.  Not a re-run of the front end: GC-frame training and connector edges are those of the full ORF set."""
        return self._resolve(self.L.phx_reannotate_flat, "phx_reannotate_flat", (self._orf_mask(forbid),), solve_all, False)

    def _orf_mask(self, sets):
        """One byte per ORF of the batch from one index array (or None) per contig."""
        n = self.n
        if len(sets) != n:
            raise ValueError("one index array (or None) per contig of the batch")
        oo = self.orf_offsets()
        mask = np.zeros(max(int(oo[n]), 1), np.uint8)
        for i, f in enumerate(sets):
            if f is None:
                continue
            idx = np.asarray(f, np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= oo[i + 1] - oo[i]):
                raise IndexError("contig %d has %d ORFs" % (i, oo[i + 1] - oo[i]))
            mask[oo[i] + idx] = 1
        return mask

    def _resolve(self, fn, name, arrays, solve_all, with_unmet):
        """The size query and the fill of one re-annotation entry point: fn(handle, *arrays, orf offsets, flags, genes, capacity, offsets,
        status, delta[, unmet], total).  Returns (status, offsets, genes, delta[, unmet]) cut to the batch."""
        head = tuple(_vp(a) for a in arrays) + (_vp(self.orf_offsets()), 1 if solve_all else 0)
        return self._genes_flat(fn, name, head, self.n, with_unmet)

    def _genes_flat(self, fn, name, head, count, with_unmet):
        """_query_fill for the entry points that deliver gene lists: (status, offsets, genes, delta[, unmet]) of `count` entries."""
        ent, offs, (genes,) = self._query_fill(fn, name, head, count, (_lib.GENE_DT,), "rc", (np.int32, np.float64) + ((np.int32,) if with_unmet else ()))
        return (ent[0], offs, genes) + tuple(ent[1:])

    def constrain(self, forbid=None, require=None, solve_all=False):
        """(status int32[n], offsets int64[n+1], genes structured array[total], delta float64[n], unmet int32[n]): the batch last run
        annotated again without the ORFs of `forbid` and keeping those of `require` — each one array of indices into orfs(i) per contig,
        or None — on the resident device graph (phx_constrain_flat).  The result calls as many required ORFs as can be
        called together and is the best such annotation; unmet[i] counts the required ORFs of contig i it does not call (all of them where
        there is no result); delta[i] = float(W(P) - D) / 1000.  A cycle through a required ORF's edge gives status 2 without genes.  An
        ORF in both sets raises PhxError (PHX_E_ARG).  With nothing required it is reannotate(forbid)."""
        n = self.n
        fmask = self._orf_mask([None] * n if forbid is None else forbid)
        rmask = self._orf_mask([None] * n if require is None else require)
        return self._resolve(self.L.phx_constrain_flat, "phx_constrain_flat", (fmask, rmask), solve_all, True)

    def _bias_array(self, bias, oo):
        """One int64 per ORF of the batch from evidence()'s `bias`: B = math.trunc(b * 1000.0) per listed ORF, summed over repeats."""
        n = self.n
        if len(bias) != n:
            raise ValueError("one dict or sequence of (ORF index, bias) pairs (or None) per contig of the batch")
        B = np.zeros(max(int(oo[n]), 1), np.int64)
        for i, pairs in enumerate(bias):
            for k, units in self._bias_pairs(i, pairs, oo[i + 1] - oo[i]):
                B[oo[i] + k] += units
        if np.abs(B).max() > 1 << 52:
            raise ValueError("a bias beyond 2^52 / 1000 SCORE units")
        return B

    def evidence(self, bias, forbid=None, solve_all=False):
        """(status int32[n], offsets int64[n+1], genes structured array[total], delta float64[n]), as reannotate() returns them: the batch
        last run annotated again with a bonus or a penalty on chosen ORFs (phx_evidence_flat).  `bias` holds, per contig,
        None or a dict or sequence of (index into orfs(i), b) pairs, b a float in SCORE units: negative is support, positive is doubt.  The
        solver adds B = math.trunc(b * 1000.0) to the ORF's edge (its units are 1/1000 of a SCORE unit, so what b holds beyond three
        decimals is cut off, towards zero); an ORF listed twice gets the sum of its B.  `forbid` is reannotate()'s.  delta[i] =
        float(D_B - D) / 1000 may be negative.  Bonuses that make a cycle negative give status -9 without genes.  A non-finite b or
        |B| > 2^52 raises ValueError.  With no bias at all it is reannotate(forbid)."""
        n = self.n
        fmask = self._orf_mask([None] * n if forbid is None else forbid)
        B = self._bias_array(bias, self.orf_offsets())
        return self._resolve(self.L.phx_evidence_flat, "phx_evidence_flat", (B, fmask), solve_all, False)

    def curate(self, bias=None, forbid=None, require=None, solve_all=False):
        """(status int32[n], offsets int64[n+1], genes structured array[total], delta float64[n], unmet int32[n]), as constrain() returns
        them: the batch last run annotated again keeping the ORFs of `require`, without those of `forbid`, and with evidence()'s `bias` on
        chosen ORFs, all in one solve (phx_curate_flat).  The result calls as many required ORFs as can be called together
        and, among those annotations, is the best under the biased weights; an ORF may be required and biased, a refused ORF's bias is
        ignored.  delta[i] = float(S(P) - D) / 1000 may be negative; unmet[i] as in constrain().  A cycle through a required ORF's edge, or
        one that the biases make negative, gives status -9 without genes.  An ORF in both sets raises PhxError (PHX_E_ARG); a bad bias
        raises as in evidence().  Without a bias it is constrain(forbid, require), without a required set evidence(bias, forbid)."""
        n = self.n
        fmask = self._orf_mask([None] * n if forbid is None else forbid)
        rmask = self._orf_mask([None] * n if require is None else require)
        B = self._bias_array([None] * n if bias is None else bias, self.orf_offsets())
        return self._resolve(self.L.phx_curate_flat, "phx_curate_flat", (B, fmask, rmask), solve_all, True)

    # ---- scenario batches ----
    @staticmethod
    def _scenario_arrays(scen, n, oo):
        """(contig int32[S], off int64[S+1], orf int32[P]) of a sequence of (contig, index array); IndexError / ValueError as _orf_mask."""
        S = len(scen)
        contig = np.zeros(max(S, 1), np.int32)
        off = np.zeros(S + 1, np.int64)
        lists = []
        for j, item in enumerate(scen):
            try:
                i, f = item
            except (TypeError, ValueError):
                raise ValueError("a scenario is a (contig, index array) pair") from None
            i = int(i)
            if i < 0 or i >= n:
                raise IndexError("scenario %d names contig %d of a batch of %d" % (j, i, n))
            idx = np.zeros(0, np.int64) if f is None else np.asarray(f, np.int64).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= oo[i + 1] - oo[i]):
                raise IndexError("contig %d has %d ORFs" % (i, oo[i + 1] - oo[i]))
            contig[j] = i
            off[j + 1] = off[j] + idx.size
            lists.append(idx)
        orf = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
        return contig, off, np.ascontiguousarray(orf if orf.size else np.zeros(1, np.int32))

    def scenarios(self, scen):
        """(status int32[S], offsets int64[S+1], genes structured array[total], delta float64[S]): S masked re-annotations of the batch
        last run in one call (phx_scenarios_flat).  `scen` is a sequence of (contig, array of indices into orfs(contig)); scenario j is
        reannotate() of that contig without exactly those ORFs — status[j], delta[j] and genes[offsets[j]:offsets[j+1]] are byte for
        byte that call's for the contig — solved side by side on the resident graph, one workgroup per scenario.  Scenarios are
        independent: the same contig may be named many times, lists may overlap, be empty (the device path) or hold duplicates."""
        n = self.n
        oo = self.orf_offsets()
        contig, off, orf = self._scenario_arrays(scen, n, oo)
        S = len(scen)
        return self._genes_flat(self.L.phx_scenarios_flat, "phx_scenarios_flat", (S, _vp(contig), _vp(off), _vp(orf), _vp(oo), 0), S, False)

    def scenarios_ms(self):
        """Device time of the last scenario solve (scenarios(), pinned_scenarios(), evidence_scenarios() or curate_scenarios()) in ms, summed over its chunks: slot records + bitmaps, masked solve, path + genes + copy
        (phx_scenarios_ms)."""
        return self._ms("phx_scenarios_ms")

    def scenario_chunks(self):
        """Chunks the last scenario solve was split into under the device-memory budget (phx_scenario_chunks)."""
        return int(self.L.phx_scenario_chunks(self.h))

    def scenario_path(self, j, contig):
        """(path as device node ids, its length D_F as a python int) of scenario j of the last scenarios(), pinned_scenarios(), evidence_scenarios() or curate_scenarios()
        call, like reannotated_path (a scenario with required ORFs: the W-sum W(P); one with biased ORFs: D_B; one with both: S(P)); `contig` is the scenario's contig.  Served while the scenario's
        chunk is resident (phx_tap_scenario_path)."""
        return self._tap_path(self.L.phx_tap_scenario_path, "phx_tap_scenario_path", self.globals(contig), int(j))

    def start_drops(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.START_DT, scen_offsets int64[total+1], genes):
        for every record of drop_margins() (same order, offsets and statuses) the best annotation when the called gene's own start ORF
        is refused while the other starts of its stop stay allowed — one scenario per called gene, all in one scenarios() call.
        drop = the scenario's delta (+inf: no path remains); restart = the index in orfs(i) of the ORF of the same stop and strand the
        new annotation calls, -1 when the stop is no longer called; genes[scen_offsets[k]:scen_offsets[k+1]] is record k's full new
        annotation."""
        st, offs, drec = self.drop_margins()
        n = self.n
        scen = []
        for i in range(n):
            for r in drec[offs[i]:offs[i + 1]]:
                scen.append((i, [self.orf_index(i, r["left"], r["right"], r["strand"])]))
        sstat, soffs, genes, delta = self.scenarios(scen)
        rec = np.zeros(len(scen), _lib.START_DT)
        k = 0
        for i in range(n):
            for r in drec[offs[i]:offs[i + 1]]:
                o = rec[k]
                o["left"], o["right"], o["strand"] = r["left"], r["right"], r["strand"]
                o["orf"] = scen[k][1][0]
                o["drop"] = delta[k]
                o["status"] = sstat[k]
                o["restart"] = -1
                fwd = r["strand"] > 0
                for g in genes[soffs[k]:soffs[k + 1]]:  # the gene of the same stop and strand, if the new annotation still calls the stop
                    if abs(int(g["frame"])) <= 3 and (g["strand"] > 0) == fwd and (g["right"] == r["right"] if fwd else g["left"] == r["left"]):
                        o["restart"] = self.orf_index(i, g["left"], g["right"], g["strand"])
                        o["restart_left"], o["restart_right"] = g["left"], g["right"]
                        break
                k += 1
        return st, offs, rec, soffs, genes

    # ---- pinned scenario batches ----
    @staticmethod
    def _pinned_scenario_arrays(scen, n, oo):
        """(contig int32[S], forbid_off int64[S+1], forbid_orf int32[], require_off int64[S+1], require_orf int32[]) of a sequence of
        (contig, forbid, require) — index arrays or None; IndexError / ValueError as _scenario_arrays."""
        try:
            triples = [(i, f, r) for i, f, r in scen]
        except (TypeError, ValueError):
            raise ValueError("a pinned scenario is a (contig, forbid, require) triple") from None
        contig, foff, forf = Annotator._scenario_arrays([(i, f) for i, f, _ in triples], n, oo)
        _, roff, rorf = Annotator._scenario_arrays([(i, r) for i, _, r in triples], n, oo)
        return contig, foff, forf, roff, rorf

    def pinned_scenarios(self, scen):
        """(status int32[S], offsets int64[S+1], genes structured array[total], delta float64[S], unmet int32[S]): S pinned
        re-annotations of the batch last run in one call (phx_pinned_scenarios_flat).  `scen` is a sequence of (contig,
        forbid, require), each list an array of indices into orfs(contig) or None; scenario j is constrain() of that contig with exactly
        those two sets — status[j], delta[j], unmet[j] and genes[offsets[j]:offsets[j+1]] are byte for byte that call's for the contig —
        solved side by side on the resident graph, one workgroup per scenario.  Scenarios are independent (the same contig may be named
        many times, lists may overlap between scenarios, be empty or hold duplicates); an ORF in both lists of one scenario raises
        PhxError (PHX_E_ARG).  As in constrain(), a required ORF whose edge lies on a cycle the source reaches gives status -9
        (PHX_S_NEGCYCLE) without genes — not rare among short overlapping ORFs; refusing an edge of the cycle takes it away.  A scenario
        that requires nothing is scenarios()' scenario."""
        n = self.n
        oo = self.orf_offsets()
        scen = list(scen)
        contig, foff, forf, roff, rorf = self._pinned_scenario_arrays(scen, n, oo)
        S = len(scen)
        head = (S, _vp(contig), _vp(foff), _vp(forf), _vp(roff), _vp(rorf), _vp(oo), 0)
        return self._genes_flat(self.L.phx_pinned_scenarios_flat, "phx_pinned_scenarios_flat", head, S, True)

    def alt_starts(self, max_alts=None):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.ALT_DT, scen_offsets int64[total+1], genes):
        for every record of drop_margins() (the called CDS genes in path order; status as drop_margins() reports it) and every OTHER ORF
        of the gene's stop group, in the order of orfs(i) (at most max_alts per gene when given), the best annotation that keeps that ORF
        — one pinned scenario each, requiring the alternative and refusing nothing, all in one pinned_scenarios() call.  The records of
        contig i are records[offsets[i]:offsets[i+1]]; delta = the scenario's delta (the alternative's margin bit for bit where status
        and unmet are 0), status -9 where the alternative's edge lies on a cycle, unmet 1 where the alternative cannot be called (no
        edge, or on no source-to-target path); n_removed / n_added count the genes of the run's annotation (the device path's) missing
        from the new one and the reverse; genes[scen_offsets[k]:scen_offsets[k+1]] is record k's full new annotation."""
        st, doffs, drec = self.drop_margins()
        n = self.n
        scen, head = [], []
        offs = np.zeros(n + 1, np.int64)
        for i in range(n):
            if doffs[i + 1] > doffs[i]:
                group = self.orfs(i)["group"]
            for r in drec[doffs[i]:doffs[i + 1]]:
                k = self.orf_index(i, r["left"], r["right"], r["strand"])
                alts = [int(a) for a in np.nonzero(group == group[k])[0] if a != k]
                for a in alts if max_alts is None else alts[: max(int(max_alts), 0)]:
                    scen.append((i, None, [a]))
                    head.append((i, r, k, a))
            offs[i + 1] = len(scen)
        sstat, soffs, genes, delta, unmet = self.pinned_scenarios(scen)
        _, roffs, rgenes = self._device_lists()
        rec = np.zeros(len(scen), _lib.ALT_DT)
        changes = self._gene_changes([h[0] for h in head], roffs, rgenes, soffs, genes)
        for x, ((i, r, k, a), (have, new, orfs_of, n_removed, n_added)) in enumerate(zip(head, changes)):
            o = rec[x]
            o["left"], o["right"], o["strand"], o["orf"], o["alt"] = r["left"], r["right"], r["strand"], k, a
            ao = orfs_of[a]
            fwd = ao["frame"] > 0
            o["alt_left"], o["alt_right"] = (ao["start"], ao["stop"] + 2) if fwd else (ao["stop"], ao["start"] + 2)
            o["status"], o["delta"], o["unmet"] = sstat[x], delta[x], unmet[x]
            o["n_removed"], o["n_added"] = n_removed, n_added
        return st, offs, rec, soffs, genes

    # ---- evidence scenario batches ----
    @staticmethod
    def _bias_units(i, k, b):
        """B = math.trunc(b * 1000.0) of evidence(), with its refusals."""
        import math

        b = float(b)
        if not math.isfinite(b) or abs(b) * 1000.0 >= 2.0 ** 60:
            raise ValueError("contig %d, ORF %d: the bias %r is not a finite number of SCORE units within 2^52 / 1000" % (i, k, b))
        return math.trunc(b * 1000.0)

    @staticmethod
    def _bias_pairs(i, pairs, n_orf):
        """(ORF index, B) for every pair of contig i's `bias` as evidence() takes it — None, a dict or a sequence of (index, b) —, in the
        order given: IndexError for an ORF the contig does not have, ValueError as _bias_units."""
        for k, b in (() if pairs is None else pairs.items() if hasattr(pairs, "items") else pairs):
            k = int(k)
            if not 0 <= k < n_orf:
                raise IndexError("contig %d has %d ORFs" % (i, n_orf))
            yield k, Annotator._bias_units(i, k, b)

    @staticmethod
    def _scenario_bias_arrays(items, oo):
        """(bias_off int64[S+1], bias_orf int32[], bias_val int64[]) of a sequence of (contig — checked by _scenario_arrays —, bias): the
        pairs as given (the library merges them); IndexError and ValueError as _bias_pairs, ValueError for a summed |B| > 2^52."""
        boff = np.zeros(len(items) + 1, np.int64)
        borf, bval = [], []
        for j, (i, pairs) in enumerate(items):
            i = int(i)
            sums = {}
            for k, B in Annotator._bias_pairs(i, pairs, oo[i + 1] - oo[i]):
                sums[k] = sums.get(k, 0) + B
                borf.append(k)
                bval.append(B)
            if any(abs(v) > 1 << 52 for v in sums.values()):
                raise ValueError("a bias beyond 2^52 / 1000 SCORE units")
            boff[j + 1] = len(borf)
        return boff, np.ascontiguousarray(borf if borf else [0], np.int32), np.ascontiguousarray(bval if bval else [0], np.int64)

    def evidence_scenarios(self, scen):
        """(status int32[S], offsets int64[S+1], genes structured array[total], delta float64[S]): S evidence-weighted re-annotations of
        the batch last run in one call (phx_evidence_scenarios_flat).  `scen` is a sequence of (contig, bias, forbid):
        `bias` what evidence() takes for one contig — None, or a dict or sequence of (index into orfs(contig), b) pairs, b a float in SCORE
        units, B = math.trunc(b * 1000.0), an ORF listed twice gets the sum of its B —, `forbid` an array of indices or None.  Scenario j
        is evidence(..., solve_all=True) of that contig with exactly that bias and that refused set — status[j], delta[j] and
        genes[offsets[j]:offsets[j+1]] are byte for byte that call's for the contig — solved side by side on the resident graph, one
        workgroup per scenario.  Scenarios are independent (the same contig may be named many times, lists may overlap, be empty or hold
        duplicates); one without a bias is scenarios()' scenario.  IndexError and ValueError as evidence()."""
        n = self.n
        oo = self.orf_offsets()
        try:
            triples = [(i, b, f) for i, b, f in scen]
        except (TypeError, ValueError):
            raise ValueError("an evidence scenario is a (contig, bias, forbid) triple") from None
        contig, foff, forf = self._scenario_arrays([(i, f) for i, _, f in triples], n, oo)
        S = len(triples)
        boff, borf, bval = self._scenario_bias_arrays([(i, b) for i, b, _ in triples], oo)
        head = (S, _vp(contig), _vp(foff), _vp(forf), _vp(boff), _vp(borf), _vp(bval), _vp(oo), 0)
        return self._genes_flat(self.L.phx_evidence_scenarios_flat, "phx_evidence_scenarios_flat", head, S, False)

    def evidence_scan(self, hits):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.EVSCAN_DT, scen_offsets int64[total+1], genes):
        `hits` holds, per contig, None or a sequence of (index into orfs(i), b) pairs as evidence() takes them; every pair is taken on its
        own — one scenario that biases that ORF alone and refuses nothing — and all run in one evidence_scenarios() call.  The records of
        contig i are records[offsets[i]:offsets[i+1]], in the order of its pairs; status[i] is the run's verdict for the contig.  A
        record holds the ORF (its index and its ends as a gene's), the bias as given, status and delta of its scenario, was_called /
        called (the ORF among the run's device genes / among the new ones) and n_removed / n_added as alt_starts() counts them;
        genes[scen_offsets[k]:scen_offsets[k+1]] is record k's full new annotation."""
        n = self.n
        if len(hits) != n:
            raise ValueError("one sequence of (ORF index, bias) pairs (or None) per contig of the batch")
        scen, head = [], []
        offs = np.zeros(n + 1, np.int64)
        for i, pairs in enumerate(hits):
            for k, b in (() if pairs is None else pairs.items() if hasattr(pairs, "items") else pairs):
                scen.append((i, [(int(k), b)], None))
                head.append((i, int(k), float(b)))
            offs[i + 1] = len(scen)
        sstat, soffs, genes, delta = self.evidence_scenarios(scen)
        st, roffs, rgenes = self._device_lists()
        rec = np.zeros(len(scen), _lib.EVSCAN_DT)
        changes = self._gene_changes([h[0] for h in head], roffs, rgenes, soffs, genes)
        for x, ((i, k, b), (have, new, orfs_of, n_removed, n_added)) in enumerate(zip(head, changes)):
            o = rec[x]
            ao = orfs_of[k]
            fwd = ao["frame"] > 0
            o["left"], o["right"] = (ao["start"], ao["stop"] + 2) if fwd else (ao["stop"], ao["start"] + 2)
            o["strand"], o["orf"], o["bias"] = (1 if fwd else -1), k, b
            o["status"], o["delta"] = sstat[x], delta[x]
            me = (int(o["left"]), int(o["right"]), bool(fwd))
            o["was_called"] = int(any((g[0], g[1], g[2] > 0) == me and abs(g[3]) <= 3 for g in have))
            o["called"] = int(any((g[0], g[1], g[2] > 0) == me and abs(g[3]) <= 3 for g in new))
            o["n_removed"], o["n_added"] = n_removed, n_added
        return np.asarray(st[:n], np.int32), offs, rec, soffs, genes

    # ---- combined scenario batches ----
    def curate_scenarios(self, scen):
        """(status int32[S], offsets int64[S+1], genes structured array[total], delta float64[S], unmet int32[S]), as pinned_scenarios()
        returns them: S combined re-annotations of the batch last run in one call (phx_curate_scenarios_flat).  `scen` is a
        sequence of (contig, bias, forbid, require): `bias` what evidence_scenarios() takes, `forbid` and `require` arrays of indices into
        orfs(contig) or None.  Scenario j is curate(..., solve_all=True) of that contig with exactly that bias and those two sets —
        status[j], delta[j], unmet[j] and genes[offsets[j]:offsets[j+1]] are byte for byte that call's for the contig — solved side by
        side on the resident graph, one workgroup per scenario.  Scenarios are independent; one without a bias is pinned_scenarios()'
        scenario, one without required ORFs evidence_scenarios()', one with neither scenarios()'.  An ORF in both sets of one scenario
        raises PhxError (PHX_E_ARG); IndexError and ValueError as evidence_scenarios() and pinned_scenarios()."""
        n = self.n
        oo = self.orf_offsets()
        try:
            quads = [(i, b, f, r) for i, b, f, r in scen]
        except (TypeError, ValueError):
            raise ValueError("a combined scenario is a (contig, bias, forbid, require) quadruple") from None
        contig, foff, forf = self._scenario_arrays([(i, f) for i, _, f, _ in quads], n, oo)
        _, roff, rorf = self._scenario_arrays([(i, r) for i, _, _, r in quads], n, oo)
        S = len(quads)
        boff, borf, bval = self._scenario_bias_arrays([(i, b) for i, b, _, _ in quads], oo)
        head = (S, _vp(contig), _vp(foff), _vp(forf), _vp(roff), _vp(rorf), _vp(boff), _vp(borf), _vp(bval), _vp(oo), 0)
        return self._genes_flat(self.L.phx_curate_scenarios_flat, "phx_curate_scenarios_flat", head, S, True)

    def curated_scan(self, hits, forbid=None, require=None):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.CUSCAN_DT, scen_offsets int64[total+1], genes,
        base_offsets int64[n+1]): evidence_scan() under pins.  `hits` holds, per contig, what evidence_scan() takes; `forbid` and `require`
        hold, per contig, what curate() takes.  For every contig with hits there is one baseline scenario — no bias, the contig's two sets
        — and one scenario per hit — that ORF biased alone under the same two sets —, all in one curate_scenarios() call.  A record is
        evidence_scan()'s plus unmet and the baseline's status, delta and unmet; was_called, n_removed and n_added are taken against the
        BASELINE's genes ("given my pins, does this hit change the call"), delta stays relative to the run.
        genes[scen_offsets[k]:scen_offsets[k+1]] is record k's full new annotation and genes[base_offsets[i]:base_offsets[i+1]] the
        baseline annotation of contig i (empty for a contig without hits): the baselines' lists follow the records' in `genes`."""
        n = self.n
        if len(hits) != n or (forbid is not None and len(forbid) != n) or (require is not None and len(require) != n):
            raise ValueError("one sequence of (ORF index, bias) pairs and one index array per set (or None) per contig of the batch")
        sets = lambda i: (None if forbid is None else forbid[i], None if require is None else require[i])
        scen, head = [], []
        offs = np.zeros(n + 1, np.int64)
        for i, pairs in enumerate(hits):
            for k, b in (() if pairs is None else pairs.items() if hasattr(pairs, "items") else pairs):
                scen.append((i, [(int(k), b)]) + sets(i))
                head.append((i, int(k), float(b)))
            offs[i + 1] = len(scen)
        total = len(scen)
        base_of = np.full(n, -1, np.int64)  # the contig's baseline scenario: behind the records', in contig order
        for i in range(n):
            if offs[i + 1] > offs[i]:
                base_of[i] = len(scen)
                scen.append((i, None) + sets(i))
        sstat, soffs, genes, delta, unmet = self.curate_scenarios(scen)
        st = self._device_lists()[0]
        boffs = np.zeros(n + 1, np.int64)
        boffs[0] = soffs[total]
        for i in range(n):
            boffs[i + 1] = soffs[base_of[i] + 1] if base_of[i] >= 0 else boffs[i]
        key = lambda g: (int(g["left"]), int(g["right"]), int(g["strand"]), int(g["frame"]))
        rec = np.zeros(total, _lib.CUSCAN_DT)
        have, have_of, orfs_of = None, -1, None
        for x, (i, k, b) in enumerate(head):
            if have_of != i:
                have, have_of, orfs_of = {key(g) for g in genes[boffs[i]:boffs[i + 1]]}, i, self.orfs(i)
            new = {key(g) for g in genes[soffs[x]:soffs[x + 1]]}
            o = rec[x]
            ao = orfs_of[k]
            fwd = ao["frame"] > 0
            o["left"], o["right"] = (ao["start"], ao["stop"] + 2) if fwd else (ao["stop"], ao["start"] + 2)
            o["strand"], o["orf"], o["bias"] = (1 if fwd else -1), k, b
            o["status"], o["delta"], o["unmet"] = sstat[x], delta[x], unmet[x]
            me = (int(o["left"]), int(o["right"]), bool(fwd))
            o["was_called"] = int(any((g[0], g[1], g[2] > 0) == me and abs(g[3]) <= 3 for g in have))
            o["called"] = int(any((g[0], g[1], g[2] > 0) == me and abs(g[3]) <= 3 for g in new))
            o["n_removed"], o["n_added"] = len(have - new), len(new - have)
            o["base_status"], o["base_delta"], o["base_unmet"] = sstat[base_of[i]], delta[base_of[i]], unmet[base_of[i]]
        return np.asarray(st[:n], np.int32), offs, rec, np.ascontiguousarray(soffs[: total + 1]), genes, boffs

    def reannotated_path(self, i):
        """(path as device node ids, its length as a python int) of contig i in the last re-annotation, constrain(), evidence() or curate(), like
        path(i): D_F, the W-sum W(P) after constrain(), D_B after evidence(), S(P) after curate()."""
        return self._tap_path(self.L.phx_tap_repath, "phx_tap_repath", self.globals(i), i)

    def remargins(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.MARGIN_DT), as margins() returns them: the path
        margin of every CDS ORF on the graph of the last reannotate() or evidence() (or constrain() without required ORFs) of the batch
        last run (phx_remargins_flat).  margin = float(d_s'(u) + W + B + d_t'(v) - D') / 1000 on the refused / biased graph:
        0 for the ORFs the re-annotation calls, the smallest further bonus that gets an uncalled ORF called, +inf with through = 0 for a
        refused ORF and where no path runs through the ORF.  called = 1 for the genes the re-annotation returned.  A contig that was not
        solved again has the records of margins().  PhxError (PHX_E_STATE) without a re-annotation of this run and after constrain()
        with required ORFs."""
        (status,), offs, (rec,) = self._query_fill(self.L.phx_remargins_flat, "phx_remargins_flat", (), self.n, (_lib.MARGIN_DT,))
        return status, offs, rec

    def remargins_ms(self):
        """Device time of the last re-annotation margins in ms: apply, conditioned reverse pass, records, copy to the host (phx_remargins_ms)."""
        return self._ms("phx_remargins_ms")

    def redrops(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.DROP_DT), as drop_margins() returns them: the
        drop margin of every CDS gene of the last reannotate() or evidence() (or constrain() without required ORFs) of the batch last
        run, in path order (phx_redrops_flat).  drop = float(D'_{-g} - D') / 1000 on the refused / biased graph: how much
        worse the best annotation under the same mask and evidence becomes when nothing is called at the gene's stop — the delta
        evidence() reports with the gene's whole stop group refused as well, minus the re-annotation's own; bypass = 0 and +inf when no
        path avoids the stop.  called = 1 for the genes the re-annotation returned.  A contig that was not solved again has the records
        of drop_margins().  PhxError (PHX_E_STATE) without a re-annotation of this run and after constrain() with required ORFs."""
        (status,), offs, (rec,) = self._query_fill(self.L.phx_redrops_flat, "phx_redrops_flat", (), self.n, (_lib.DROP_DT,))
        return status, offs, rec

    def redrops_ms(self):
        """Device time of the last re-annotation drop margins in ms: trees + labels, candidates, fixups, copy to the host (phx_redrops_ms)."""
        return self._ms("phx_redrops_ms")

    def reprofile(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.PROFILE_DT), as profile() returns them: the coding
        profile of every contig on the graph of the last reannotate() or evidence() (or constrain() without required ORFs) of the batch
        last run (phx_reprofile_flat).  fwd / rev / gap of a slot: the minimum over the forward gene edges / reverse gene
        edges / connectors that cover it of float(d_s'(u) + W + B + d_t'(v) - D') / 1000 on the refused / biased graph — now that this
        evidence is in, what it costs the best annotation under it to have the stretch inside a forward gene, inside a reverse gene, or
        between genes; a refused ORF's edge takes no part.  A contig that was not solved again has the records of profile().  PhxError
        (PHX_E_STATE) without a re-annotation of this run and after constrain() with required ORFs."""
        (status,), offs, (rec,) = self._query_fill(self.L.phx_reprofile_flat, "phx_reprofile_flat", (), self.n, (_lib.PROFILE_DT,))
        return status, offs, rec

    def reprofile_ms(self):
        """Device time of the last re-annotation profiles in ms: candidates + tables + push-down, the slots' bounds, copy to the host (phx_reprofile_ms)."""
        return self._ms("phx_reprofile_ms")

    def pinprofile(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.PROFILE_DT, lost int32[total, 3]): reprofile()
        for every re-annotation of the batch last run, constrain() and curate() with required ORFs included (phx_pinprofile_flat,
        DESIGN.md §37).  For a contig solved with required ORFs every edge has Delta'' = lost * M + s as pinmargins() decodes it, and a
        slot's fwd / rev / gap is float(s) / 1000 of the lexicographic minimum of (lost, s) over the forward gene edges / reverse gene
        edges / connectors that cover it, lost[k] = (fwd, rev, gap) the kept required ORFs that minimum gives up — now that these genes
        are pinned, what the stretch costs as forward gene, as reverse gene or as gap, and how many pins that would give up.  A value may
        be negative where lost > 0; the order is (lost, value) >= (0, 0.0), which one track of every slot of a solved contig has.  +inf
        with lost 0 where nothing of the track covers the slot.  Elsewhere the records are reprofile()'s (profile()'s for a contig that
        was not solved again) and lost is 0.  PhxError (PHX_E_STATE) only without a re-annotation of this run."""
        (status,), offs, (rec, lost) = self._query_fill(self.L.phx_pinprofile_flat, "phx_pinprofile_flat", (), self.n, (_lib.PROFILE_DT, np.dtype((np.int32, (3,)))), "rrc")
        return status, offs, rec, lost.reshape(-1, 3)

    def pinprofile_ms(self):
        """Device time of the last pinned profiles in ms: candidates + tables + push-down over every round, the slots' bounds, copy to the host (phx_pinprofile_ms)."""
        return self._ms("phx_pinprofile_ms")

    def pinprofile_stats(self):
        """Counters of the last pinned profiles (phx_pinprofile_stats): the contigs the pinned kernels covered, the table rounds they ran (3
        per contig and one more per distinct lost > 0 among a track's slots), the slots with lost > 0 on any track."""
        out = (C.c_int64 * 3)()
        self._chk(self.L.phx_pinprofile_stats(self.h, out), "phx_pinprofile_stats")
        return dict(zip(("contigs", "rounds", "lost_slots"), [int(x) for x in out]))

    def redrop_stats(self):
        """drop_stats() of the last re-annotation drop margins, over the contigs that were solved again (phx_redrop_stats)."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.phx_redrop_stats(self.h, out), "phx_redrop_stats")
        return dict(zip(("slots", "cross", "rescanned", "layered"), [int(x) for x in out]))

    def rereplacements(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.REPL_DT, genes structured array of _lib.GENE_DT),
        as replacements() returns them: for every record of redrops() (same order, statuses and offsets; drop, called and bypass
        bit-equal) what the best path under the same mask and evidence calls instead when nothing is called at the gene's stop
        (phx_rereplacements_flat).  The removed genes are genes of the re-annotation, the scores the ORFs' weights without
        the bias.  A contig that was not solved again has the records of replacements().  PhxError (PHX_E_STATE) as redrops()."""
        (status,), offs, (rec, genes) = self._query_fill(self.L.phx_rereplacements_flat, "phx_rereplacements_flat", (), self.n, (_lib.REPL_DT, _lib.GENE_DT), "rcrc")
        return status, offs, rec, genes

    def rereplacement_path(self, i, k):
        """R'_g of record k of contig i (rereplacements()[2][offsets[i] + k]): device node ids, source first, the re-annotation's path
        (reannotated_path(i)) around the detour; empty when bypass = 0.  A contig that was not solved again gives replacement_path(i, k)."""
        n = C.c_int32()
        self._chk(self.L.phx_tap_rereplacement(self.h, i, k, None, 0, C.byref(n)), "phx_tap_rereplacement")
        p = np.zeros(max(n.value, 1), np.int32)
        self._chk(self.L.phx_tap_rereplacement(self.h, i, k, p.ctypes.data_as(C.c_void_p), len(p), C.byref(n)), "phx_tap_rereplacement")
        return p[: n.value].copy()

    def rereplacements_ms(self):
        """Device time of the last re-annotation replacements in ms: argmin, walk + genes, copy to the host (phx_rereplacements_ms)."""
        return self._ms("phx_rereplacements_ms")

    def rereplacement_stats(self):
        """replacement_stats() of the last re-annotation replacements, over the contigs that were solved again (phx_rereplacement_stats)."""
        out = (C.c_int64 * 5)()
        self._chk(self.L.phx_rereplacement_stats(self.h, out), "phx_rereplacement_stats")
        return dict(zip(("cross", "chain_nodes", "cross_kept", "cut", "regrown"), [int(x) for x in out]))

    def redist(self, i, to_target=False):
        """Exact distances of every node of contig i on the last re-annotation's graph as python ints (None: unreached), device node
        order: d_s' from the source, or with to_target d_t' to the target within the nodes the re-solve reached (phx_tap_redist).  A
        contig that was not solved again gives dist(i) / dist_to_target(i)."""
        return self._tap_dist(self.L.phx_tap_redist, "phx_tap_redist", i, 1 if to_target else 0)

    def pinmargins(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.MARGIN_DT, lost int32[total]): remargins() for
        every re-annotation of the batch last run, constrain() and curate() with required ORFs included (phx_pinmargins_flat, DESIGN.md
        §24).  For a contig solved with required ORFs, lost[k] is the number of kept required ORFs the best path through ORF k gives up
        and margin the change of the path sum on that path in SCORE units — it may be negative where lost > 0; the order is (lost,
        margin) >= (0, 0.0), which a called gene has.  Requiring an uncalled ORF with lost 0 as well gets it called, keeps unmet and
        raises delta by its margin.  Elsewhere the records are remargins()' and lost is 0.  PhxError (PHX_E_STATE) only without a
        re-annotation of this run."""
        (status,), offs, (rec, lost) = self._query_fill(self.L.phx_pinmargins_flat, "phx_pinmargins_flat", (), self.n, (_lib.MARGIN_DT, np.int32), "rrc")
        return status, offs, rec, lost

    def pinmargins_ms(self):
        """Device time of the last pinned margins in ms: apply, reverse pass, records, copy to the host (phx_pinmargins_ms)."""
        return self._ms("phx_pinmargins_ms")

    def pindrops(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.DROP_DT, lost int32[total]): redrops() for every
        re-annotation of the batch last run, constrain() and curate() with required ORFs included (phx_pindrops_flat).
        For a contig solved with required ORFs, lost[k] is the number of kept required ORFs the best annotation without a gene at gene
        k's stop gives up — net: a kept pin at the stop is lost, a required ORF that comes in instead counts against it — and drop the change of the path sum in SCORE units; it may
        be negative where lost > 0; the order is (lost, drop) >= (0, 0.0).  It is what curate(bias, forbid + the ORFs of the gene's stop
        group, require - them) returns, without that solve.  Elsewhere the records are redrops()' and lost is 0.  PhxError
        (PHX_E_STATE) only without a re-annotation of this run."""
        (status,), offs, (rec, lost) = self._query_fill(self.L.phx_pindrops_flat, "phx_pindrops_flat", (), self.n, (_lib.DROP_DT, np.int32), "rrc")
        return status, offs, rec, lost

    def pindrops_ms(self):
        """Device time of the last pinned drop margins in ms: trees + labels, candidates, fixups, copy to the host (phx_pindrops_ms)."""
        return self._ms("phx_pindrops_ms")

    def pindrop_stats(self):
        """drop_stats() of the last pinned drop margins, over the contigs that were solved again (phx_pindrop_stats)."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.phx_pindrop_stats(self.h, out), "phx_pindrop_stats")
        return dict(zip(("slots", "cross", "rescanned", "layered"), [int(x) for x in out]))

    def pinreplacements(self):
        """(status int32[n], offsets int64[n+1], records structured array[total] of _lib.REPL_DT, genes structured array of _lib.GENE_DT,
        lost int32[total]): rereplacements() for every re-annotation of the batch last run, constrain() and curate() with required ORFs
        included (phx_pinreplacements_flat).  For every record of pindrops() (same order, statuses and offsets; drop,
        called, bypass and lost bit-equal) what the best annotation under the same mask, evidence and pins calls instead when nothing is
        called at the gene's stop: the genes curate(bias, forbid + the ORFs of the gene's stop group, require - them) would return,
        without that solve.  Where lost > 0 the replacement carries that many kept required ORFs fewer.  Elsewhere the records are
        rereplacements()' (replacements()' for a contig that was not solved again) and lost is 0.  PhxError (PHX_E_STATE) only without a
        re-annotation of this run."""
        (status,), offs, (rec, lost, genes) = self._query_fill(self.L.phx_pinreplacements_flat, "phx_pinreplacements_flat", (), self.n,
                                                               (_lib.REPL_DT, np.int32, _lib.GENE_DT), "rrcrc")
        return status, offs, rec, genes, lost

    def pinreplacement_path(self, i, k):
        """R'_g of record k of contig i (pinreplacements()[2][offsets[i] + k]): device node ids, source first, the re-annotation's path
        (reannotated_path(i)) around the detour; empty when bypass = 0.  A contig that was not solved again gives replacement_path(i, k)."""
        n = C.c_int32()
        self._chk(self.L.phx_tap_pinreplacement(self.h, i, k, None, 0, C.byref(n)), "phx_tap_pinreplacement")
        p = np.zeros(max(n.value, 1), np.int32)
        self._chk(self.L.phx_tap_pinreplacement(self.h, i, k, p.ctypes.data_as(C.c_void_p), len(p), C.byref(n)), "phx_tap_pinreplacement")
        return p[: n.value].copy()

    def pinreplacements_ms(self):
        """Device time of the last pinned replacements in ms: argmin, walk + genes, copy to the host (phx_pinreplacements_ms)."""
        return self._ms("phx_pinreplacements_ms")

    def pinreplacement_stats(self):
        """replacement_stats() of the last pinned replacements, over the contigs that were solved again (phx_pinreplacement_stats)."""
        out = (C.c_int64 * 5)()
        self._chk(self.L.phx_pinreplacement_stats(self.h, out), "phx_pinreplacement_stats")
        return dict(zip(("cross", "chain_nodes", "cross_kept", "cut", "regrown"), [int(x) for x in out]))

    def pindist(self, i, to_target=False):
        """redist(i, to_target) for every re-annotation (phx_tap_pindist).  A contig solved with required ORFs gives per node None
        (unreached) or (S, count): the sum of W + B and the number of required ORFs on the best path from the source (to the target
        within the nodes the re-solve reached), best meaning most required ORFs first.  Any other contig gives redist()'s plain ints."""
        return self._tap_dist(self.L.phx_tap_pindist, "phx_tap_pindist", i, 1 if to_target else 0, pinned=True)

    def reannotate_ms(self):
        """Device time of the last re-annotation in ms: mask build, masked solve, path + genes + copy (phx_reannotate_ms)."""
        return self._ms("phx_reannotate_ms")

    def drop_stats(self):
        """Counters of the last drop-margins computation (phx_drop_stats): gene slots, slots with cross nodes, saturated slots rescanned
        exactly, contigs whose trees were built layer by layer."""
        out = (C.c_int64 * 4)()
        self._chk(self.L.phx_drop_stats(self.h, out), "phx_drop_stats")
        return dict(zip(("slots", "cross", "rescanned", "layered"), [int(x) for x in out]))

    # ---- solver alone (fastpathz boundary) ----
    def solve(self, V, src, dst, weights, source, target, n_limbs=None):
        """Exact shortest path over integer weights (python ints).  Returns (path node ids, distance) or ([], None)."""
        E = len(src)
        mx = max([abs(int(w)) for w in weights] + [1])
        bits = mx.bit_length() + max(V, 2).bit_length() + 3
        if n_limbs is None:
            n_limbs = 2 if bits <= 128 else 4 if bits <= 256 else 8 if bits <= 512 else 17
        wl = np.zeros((max(E, 1), n_limbs), np.uint64)
        mask = (1 << 64) - 1
        for e, w in enumerate(weights):
            w = int(w) & ((1 << (64 * n_limbs)) - 1)
            for k in range(n_limbs):
                wl[e, k] = (w >> (64 * k)) & mask
        s = np.ascontiguousarray(src, np.int32)
        d = np.ascontiguousarray(dst, np.int32)
        path = np.zeros(V, np.int32)
        n = C.c_int32()
        dl = np.zeros(n_limbs, np.uint64)
        self._chk(self.L.phx_solve(self.h, V, E, s.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), wl.ctypes.data_as(C.c_void_p),
                                   n_limbs, source, target, path.ctypes.data_as(C.c_void_p), V, C.byref(n), dl.ctypes.data_as(C.c_void_p)), "phx_solve")
        if n.value == 0:
            return [], None
        return path[: n.value].tolist(), _limbs_to_int(dl, n_limbs)

    # ---- measurement ----
    def set_profiling(self, on=True):
        self._chk(self.L.phx_set_profiling(self.h, 1 if on else 0), "phx_set_profiling")

    def set_profiling_stages(self, names):
        """Bracket only the named stages with events (two events per run for one stage); [] switches profiling off."""
        idx = {self.L.phx_stage_name(k).decode(): k for k in range(_lib.N_STAGES)}
        mask = 0
        for nm in names:
            mask |= 1 << idx[nm]
        self._chk(self.L.phx_set_profiling_stages(self.h, mask), "phx_set_profiling_stages")

    def stage_ms(self, reset=True):
        ms = (C.c_float * _lib.N_STAGES)()
        nl = (C.c_int32 * _lib.N_STAGES)()
        self._chk(self.L.phx_get_stage_ms(self.h, ms, nl, 1 if reset else 0), "phx_get_stage_ms")
        return {self.L.phx_stage_name(k).decode(): (float(ms[k]), int(nl[k])) for k in range(_lib.N_STAGES)}

    def front_runs(self):
        """Runs whose front end was the fused launch of small batches (phx_front_runs; negative: it was switched off after a stall)."""
        return int(self.L.phx_front_runs(self.h))

    def chain_runs(self):
        """Runs whose nodes, attributes, edge count and scan were one launch (phx_chain_runs)."""
        return int(self.L.phx_chain_runs(self.h))

    def seg_runs(self):
        """Runs whose 128-bit contigs were solved in segments side by side (phx_seg_runs)."""
        return int(self.L.phx_seg_runs(self.h))

    def seg_fallbacks(self):
        """Contigs, over the life of the context, whose segments could not be joined or proven and that one sweep solved in the same run."""
        return int(self.L.phx_seg_fallbacks(self.h))

    def seg_stats(self, i):
        """Per-segment records of contig i in the last run (phx_seg_stats): rows of [windows | done, status, first node, end node, ticks of 10 ns, phases, packs, step-backs]."""
        import numpy as np

        out = np.zeros((64, 8), np.int32)
        n = self.L.phx_seg_stats(self.h, int(i), out.ctypes.data_as(C.c_void_p), 64)
        return out[:n]

    def plan_timeouts(self):
        """Contigs, over the life of the context, whose shortest-path wavefront gave up waiting for the planner it was launched beside
        (include/phx.h: phx_plan_timeouts): 0 unless other contexts / processes kept the planner's wavefronts off the device."""
        return int(self.L.phx_plan_timeouts(self.h))

    def batch_sizes(self):
        v = [C.c_int64() for _ in range(4)]
        self._chk(self.L.phx_batch_sizes(self.h, *[C.byref(x) for x in v]), "phx_batch_sizes")
        return dict(L=v[0].value, n_orf=v[1].value, n_node=v[2].value, n_edge=v[3].value)
