// phx_orf.inc — k_orf, k_bit_prefix, k_orf_stats, k_score: ORF scan on the bitmaps, prefix popcounts, per-ORF statistics, weights (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// ORF scan on the codon bitmaps.  A "stop event" (forward stop codon, or the closing reverse-complement stop
// codon) owns its stop-group (orfs.py:17-32).  Work item = one 64-codon word of one (strand, frame):
// k_orf<false> counts ORFs / groups per item and turns the counts into exclusive offsets with one block
// scan; k_orf<true> re-walks the items and writes the records.  The device order of groups is therefore
// (strand, frame, codon); the reference's insertion order is kept as DGrp.evkey.
struct OrfOut {
    DOrf *orf;
    DGrp *grp;
    unsigned long long *nbF, *nbR; // node-existence bitmaps over positions: forward-strand / reverse-strand node at that key
    // node bits not yet written: the nodes a thread marks one after the other (the starts of a group, its stop, the next group of the
    // same bitmap word) mostly fall into the same 64-position word, so they are collected and go out as one atomicOr per word
    // instead of one per node (2.9 M atomics per benchmark batch were a third of k_orf<true>)
    unsigned long long *acc_nb;
    int acc_w;
    uint64_t acc_bits;
};
__device__ __forceinline__ void flush_nodes(OrfOut &o) {
    if (o.acc_bits) atomicOr(&o.acc_nb[o.acc_w], (unsigned long long)o.acc_bits);
    o.acc_bits = 0;
}
__device__ __forceinline__ void mark_node(OrfOut &o, unsigned long long *nb, int q) {
    const int w = q >> 6;
    if (w != o.acc_w || nb != o.acc_nb) { flush_nodes(o); o.acc_nb = nb; o.acc_w = w; }
    o.acc_bits |= 1ull << (q & 63);
}
struct FrameBits {
    const uint64_t *FS, *RS, *FT, *RT, *FA, *RA; // start / stop codons of either strand; codons that read 'atg' on the forward / reverse strand
    int f;    // 0-based frame = position of codon 0
    int ncod; // complete codons in this frame
};
// highest set bit with index < k, or -1
__device__ __forceinline__ int prev_bit(const uint64_t *__restrict__ B, int k) {
    if (k <= 0) return -1;
    int w = (k - 1) >> 6;
    uint64_t m = B[w] & (~0ull >> (63 - ((k - 1) & 63)));
    while (true) {
        if (m) return (w << 6) + 63 - __clzll((long long)m);
        if (--w < 0) return -1;
        m = B[w];
    }
}
__device__ __forceinline__ uint64_t range_mask(int w, int lo, int hi) { // bits of word w that lie in [lo, hi]
    uint64_t m = ~0ull;
    if ((lo >> 6) == w) m &= ~0ull << (lo & 63);
    if ((hi >> 6) == w) m &= ~0ull >> (63 - (hi & 63));
    return m;
}

// an ORF head (start, stop, frame|flags, grp) as one 16-byte store
__device__ __forceinline__ void orf_head(DOrf *r, int start, int stop, int frame, uint32_t flags, int grp) {
    static_assert(sizeof(DOrf) == 16, "ORF head");
    *(uint4 *)r = make_uint4((uint32_t)start, (uint32_t)stop, (uint32_t)(uint8_t)(int8_t)frame | (flags << 24), (uint32_t)grp);
}

// Forward group closed by the stop codon (or, for the end fragment, the last codon of the frame) k:
// functions.py:202-214 / 229-239.  Starts are emitted nearest first == reversed(starts[frame]).
template <bool EMIT>
__device__ int fwd_group(const FrameBits &F, int k, int kp /* previous stop codon of the frame, -1: none */, int dmin,
                         OrfOut &o, int obase, int gidx, int evkey) {
    const int lo = kp + 1, hi = k - dmin; // start codons ks with stop+2-start+1 >= minlen
    const int p = F.f + 3 * k;
    int n = 0, pick = -1;
    if (hi >= lo) {
        auto word = [&](int w, uint64_t m, uint64_t fa) {
            m &= range_mask(w, lo, hi);
            if (!EMIT) n += __popcll(m);
            else {
                // the heads carry (start, stop, frame, group); RBS bin, start-codon index and the 'atg' flag are per-position records that
                // k_orf_stats gathers with one thread per ORF (here every gather would sit in this thread's walk)
                const uint64_t ma = fa & m;
                if (ma) { const int j = __ffsll((long long)ma) - 1; pick = n + __popcll(m & ~((2ull << j) - 1ull)); } // the farthest 'atg' start so far: starts are emitted nearest first
                while (m) {
                    const int j = 63 - __clzll((long long)m);
                    m &= ~(1ull << j);
                    const int q = F.f + 3 * ((w << 6) + j);
                    orf_head(&o.orf[obase + n], q + 1, p + 1, F.f + 1, 0u, gidx);
                    mark_node(o, o.nbF, q);
                    n++;
                }
            }
        };
        const int wl = lo >> 6;
        for (int w = hi >> 6; w >= wl; w -= 2) { // two words per step: a long ORF is a chain of dependent loads otherwise
            const bool two = w - 1 >= wl;
            const uint64_t m0 = F.FS[w], m1 = two ? F.FS[w - 1] : 0ull;
            const uint64_t a0 = EMIT ? F.FA[w] : 0ull, a1 = (EMIT && two) ? F.FA[w - 1] : 0ull;
            word(w, m0, a0);
            if (two) word(w - 1, m1, a1);
        }
    }
    // no stop to the left: the frame opens with a pseudo-start unless its first codon is a start (functions.py:186-191)
    if (kp < 0 && !(F.FS[0] & 1ull) && hi >= 0 && k > 0) {
        if (EMIT) {
            const int q0 = F.f;
            orf_head(&o.orf[obase + n], q0 + 1, p + 1, F.f + 1, 2u /* pseudo-start */, gidx);
            mark_node(o, o.nbF, q0);
            if (F.FA[0] & 1ull) pick = n;
        }
        n++;
    }
    if (EMIT && n) {
        DGrp *g = &o.grp[gidx];
        g->stop = p + 1; g->orf_begin = obase; g->n = n; g->node = -1; g->frame = F.f + 1; g->evkey = evkey; g->pick = pick; g->pad0 = 0;
        mark_node(o, o.nbF, p);
    }
    return n;
}

// Reverse group: ORFs between the previous rc-stop of the frame (or the frame's first codon: stops =
// {-1:1,-2:2,-3:3}, functions.py:184) and the pending rc-starts, emitted when the closing rc-stop k is
// met (functions.py:215-227), or after the loop for the open group (virt: functions.py:240-251, with a
// pseudo-start on the last codon unless rev_comp(codon) is a start codon).  Starts ascend.
template <bool EMIT>
__device__ int rev_group(const FrameBits &F, const uint32_t *__restrict__ rec, const DParams *__restrict__ P, int k, int kp /* previous rc-stop of the frame, -1: none */, bool virt, int L,
                         int dmin, OrfOut &o, int obase, int gidx, int evkey) {
    const int sk = kp >= 0 ? kp : 0;
    const int lo = sk + dmin, hi = virt ? F.ncod - 1 : k - 1;
    const int psk = F.f + 3 * sk;
    int n = 0, pick = -1;
    if (hi >= lo) {
        auto word = [&](int w, uint64_t m, uint64_t ra) {
            m &= range_mask(w, lo, hi);
            if (!EMIT) n += __popcll(m);
            else {
                const uint64_t ma = ra & m;
                if (ma) { const int j = 63 - __clzll((long long)ma); pick = n + __popcll(m & ((1ull << j) - 1ull)); } // starts ascend: the last 'atg' one is the longest
                while (m) {
                    const int j = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const int sv = F.f + 3 * ((w << 6) + j);
                    orf_head(&o.orf[obase + n], sv + 1, psk + 1, -(F.f + 1), 0u, gidx);
                    mark_node(o, o.nbR, sv);
                    n++;
                }
            }
        };
        const int wh = hi >> 6;
        for (int w = lo >> 6; w <= wh; w += 2) { // two words per step, see fwd_group
            const bool two = w + 1 <= wh;
            const uint64_t m0 = F.RS[w], m1 = two ? F.RS[w + 1] : 0ull;
            const uint64_t a0 = EMIT ? F.RA[w] : 0ull, a1 = (EMIT && two) ? F.RA[w + 1] : 0ull;
            word(w, m0, a0);
            if (two) word(w + 1, m1, a1);
        }
    }
    if (virt && F.ncod - 1 >= lo) {
        const int s = F.f + 3 * (F.ncod - 1);
        // is rev_comp(last codon) a start codon (functions.py:241-242)?  The one place that asks this of a codon that need not be a
        // start of either strand: decoded from the three letters (once per frame and contig)
        const uint32_t c0 = rec_base(rec, s), c1 = rec_base(rec, s + 1), c2 = rec_base(rec, s + 2); // (rec: the contig's records)
        const uint32_t ci = ((c0 | c1 | c2) & 4u) ? 64u : ((c0 & 3u) | ((c1 & 3u) << 2) | ((c2 & 3u) << 4));
        if (!(P->cls_tab[ci] & 0x80u)) {
            if (EMIT) {
                orf_head(&o.orf[obase + n], s + 1, psk + 1, -(F.f + 1), 2u /* pseudo-start */, gidx);
                mark_node(o, o.nbR, s);
                { const int ks = F.ncod - 1; if ((F.RA[ks >> 6] >> (ks & 63)) & 1ull) pick = n; }
            }
            n++;
        }
    }
    if (EMIT && n) {
        DGrp *g = &o.grp[gidx];
        g->stop = psk + 1; g->orf_begin = obase; g->n = n; g->node = -1; g->frame = -(F.f + 1); g->evkey = evkey; g->pick = pick; g->pad0 = 0;
        mark_node(o, o.nbR, psk);
    }
    return n;
}

__device__ __forceinline__ FrameBits frame_bits(const uint64_t *bits, int nw, int f, int L) {
    FrameBits F;
    F.FS = bits + (size_t)(0 * 3 + f) * nw; F.RS = bits + (size_t)(1 * 3 + f) * nw;
    F.FT = bits + (size_t)(2 * 3 + f) * nw; F.RT = bits + (size_t)(3 * 3 + f) * nw;
    F.FA = bits + (size_t)(PHX_PLANE_ATG * 3 + f) * nw; F.RA = bits + (size_t)((PHX_PLANE_ATG + 1) * 3 + f) * nw;
    F.f = f;
    F.ncod = L - f >= 3 ? (L - f) / 3 : 0;
    return F;
}

// The counting pass is one workgroup per contig (it ends in a block scan) and is bound by the latency of its bitmap
// walks: it runs with 1024 threads so that a thread owns one or two words instead of seven.
// (a batch of short contigs — a few thousand bases, a dozen words per frame — is counted with 256 threads per contig: CT)
#define ORF_COUNT_T 1024
template <bool EMIT, int CT>
__device__ __forceinline__ void b_orf(const DBatch &b, const int bx, const int by, const int gy) {
    constexpr int T = EMIT ? NT : CT;
    if (EMIT && b.tot->overflow) return;
    __shared__ uint32_t s_scan[T / 64 + 1];
    DMeta *meta = &b.meta[bx];
    const int L = meta->L;
    if (meta->status < 0 || L < 6) {
        if (threadIdx.x == 0) {
            if (L < 6 && meta->status == 0) meta->status = PHX_S_TOOSHORT;
            meta->n_orf = 0; meta->n_grp = 0;
        }
        return;
    }
    const uint32_t *__restrict__ rec = b.recs + (size_t)meta->rec_off * REC_WORDS;
    const uint64_t *bits = b.bits + meta->bits_off;
    const int nw = meta->nw;
    uint2 *item = b.item + meta->item_off;
    const int minlen = b.params->minlen;
    const int dmin = (minlen - 1) / 3; // codons between start and stop so that the ORF length reaches minlen
    OrfOut o;
    o.orf = EMIT ? b.orf + meta->orf_off : nullptr;
    o.grp = EMIT ? b.grp + meta->grp_off : nullptr;
    o.nbF = (unsigned long long *)(b.nbits + meta->nbits_off);
    o.nbR = o.nbF + 3 * (size_t)nw;
    o.acc_nb = o.nbF; o.acc_w = 0; o.acc_bits = 0;
    const int nitems = 6 * nw;
    // count pass: one workgroup per contig (it needs the block scan); emit pass: the items are spread over
    // gy workgroups, every thread takes one item at a time (offsets are already known)
    const int nthr = EMIT ? T * (int)gy : T;
    const int gtid = EMIT ? (int)by * T + (int)threadIdx.x : (int)threadIdx.x;
    const int per = EMIT ? 1 : (nitems + T - 1) / T;
    const int ia = EMIT ? gtid : (int)threadIdx.x * per, ib = EMIT ? nitems : (ia + per < nitems ? ia + per : nitems);
    const int istep = EMIT ? nthr : 1;
    // The group of a stop codon starts after the previous stop of its frame.  For the first stop of a bitmap word that one lies in
    // an earlier word: the count pass finds, by a max-scan over the items, the last non-empty word in front of every item (iprev),
    // so that neither pass walks back through the empty words of a long ORF (one dependent load per word); the other stops of a
    // word follow the stop before them.
    int32_t *iprev = b.iprev + meta->item_off;
    uint32_t carry = 0; // 1 + index of the last non-empty item before mine (0: none)
    if (!EMIT) {
        uint32_t mine = 0;
        for (int it = ia; it < ib; it++) {
            const int sf = it / nw, w = it - sf * nw;
            if (bits[(size_t)((sf < 3 ? 2 : 3) * 3 + (sf < 3 ? sf : sf - 3)) * nw + w]) mine = (uint32_t)it + 1u;
        }
        uint32_t tot;
        carry = block_excl_max<T>(mine, s_scan, &tot);
        __syncthreads(); // s_scan is used again below
    }
    uint32_t so = 0, sg = 0;
    for (int it = ia; it < ib; it += istep) {
        const int sf = it / nw, w = it - sf * nw;
        const int s = sf / 3, f = sf - 3 * s;
        const FrameBits F = frame_bits(bits, nw, f, L);
        const uint64_t *plane = s == 0 ? F.FT : F.RT;
        uint64_t m = plane[w];
        int ip;
        if (!EMIT) { ip = (int)carry - 1; iprev[it] = ip; if (m) carry = (uint32_t)it + 1u; }
        else ip = iprev[it];
        uint32_t no = 0, ng = 0;
        uint2 base = make_uint2(0, 0);
        if (EMIT) base = item[it];
        int kp = -1;
        if (m && ip >= sf * nw) { const int wp = ip - sf * nw; kp = (wp << 6) + 63 - __clzll((long long)plane[wp]); } // same (strand, frame): a word with a stop in it
        while (m) {
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            const int k = (w << 6) + j;
            const int ev = f + 3 * k; // main-loop events are discovered in position order (functions.py:195)
            const int n = s == 0 ? fwd_group<EMIT>(F, k, kp, dmin, o, (int)(base.x + no), (int)(base.y + ng), ev)
                                 : rev_group<EMIT>(F, rec, b.params, k, kp, false, L, dmin, o, (int)(base.x + no), (int)(base.y + ng), ev);
            kp = k;
            no += (uint32_t)n;
            ng += n ? 1u : 0u;
        }
        if (!EMIT) item[it] = make_uint2(no, ng);
        else flush_nodes(o);
        so += no; sg += ng;
    }
    int run_orf, run_grp;
    if (!EMIT) {
        uint32_t tot, gtot;
        uint32_t exo = block_excl_scan<T>(so, s_scan, &tot);
        uint32_t exg = block_excl_scan<T>(sg, s_scan, &gtot);
        for (int it = ia; it < ib; it++) {
            const uint2 c = item[it];
            item[it] = make_uint2(exo, exg);
            exo += c.x; exg += c.y;
        }
        run_orf = (int)tot; run_grp = (int)gtot;
    } else {
        run_orf = meta->n_orf_main; run_grp = meta->n_grp_main;
    }
    // fragments at the right end, functions.py:229-251: frame 1 fwd, frame 1 rev, frame 2 fwd, ...
    if (threadIdx.x == 0 && by == 0) {
        if (!EMIT) { meta->n_orf_main = run_orf; meta->n_grp_main = run_grp; }
        for (int f = 0; f < 3; f++) {
            const FrameBits F = frame_bits(bits, nw, f, L);
            if (F.ncod < 1) continue;
            const int ke = F.ncod - 1;
            if (!((F.FT[ke >> 6] >> (ke & 63)) & 1ull)) { // else the main loop closed the group and starts[frame] is empty
                const int n = fwd_group<EMIT>(F, ke, prev_bit(F.FT, ke), dmin, o, run_orf, run_grp, L + 2 * f);
                run_orf += n; run_grp += n ? 1 : 0;
            }
            const int n = rev_group<EMIT>(F, rec, b.params, ke, prev_bit(F.RT, F.ncod), true, L, dmin, o, run_orf, run_grp, L + 2 * f + 1);
            run_orf += n; run_grp += n ? 1 : 0;
        }
        if (EMIT) flush_nodes(o);
        if (!EMIT) { meta->n_orf = run_orf; meta->n_grp = run_grp; }
        else if (run_orf != meta->n_orf || run_grp != meta->n_grp) meta->status = PHX_E_STATE; // cannot happen
    }
}
template <bool EMIT, int CT = ORF_COUNT_T>
__global__ __launch_bounds__(EMIT ? NT : CT) void k_orf(DBatch b) { b_orf<EMIT, CT>(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }


// ------------------------------------------------------------------------------------------------
// ORF statistics on the bit-sliced features, one thread per ORF: the 3x3 GC-frame class histogram over the sense
// codons (functions.py:286-298) is a popcount over a codon range of 9 class bitmaps, p_stop (orfs.py:162-173) a
// popcount over a position range of the a/t/g(/c) base bitmaps.  Then one thread per stop-group for the GC frame
// plot training of functions.py:261-279 (same popcounts over a sub-range of the first 'atg' ORF).
// Prefix popcounts of the bitmaps the statistics read (k_bit_prefix, one wavefront per contig and plane): the ORFs of a stop group
// are nested and the longest ones run to thousands of codons, so counting by walking the words makes a wavefront as slow as its
// longest ORF; with a record every PRE_G words a range costs two records and the few words at its ends.
//   class planes (strand, frame): record g = {popc(x0&n0), popc(x0&n1), popc(x1&n0), popc(x1&n1), popc(x0), popc(x1), popc(n0),
//     popc(n1)} over the words [0, g * PRE_G) of the four marginals x0 = max_idx==1, x1 = max_idx==2, n0 = min_idx==1,
//     n1 = min_idx==2 (combined from the strand's three comparison bitmaps, cls_counts); contig i has 6 planes of nw / PRE_G + 1
//     records, the first at record 6 * (bits_off / PHX_BITMAP_WORDS_PER_NW / PRE_G + i);
//   bases: entry g = {a, c, t, g} (unambiguous letters) over the records [0, g) of the contig's bit planes (DBatch.recs: 96 positions
//     per record), 2 nw + 2 entries per contig, the first at entry 2 * (bits_off / PHX_BITMAP_WORDS_PER_NW) + 2 i.
struct ClsPre { uint32_t j00, j01, j10, j11, x0, x1, n0, n1; };
static_assert(sizeof(ClsPre) == 32, "class prefix record");
// (A, B, C) = the comparison planes a > b, b > c, a > c of k_features: max_idx == 1 is A & C, == 2 is ~A & B, min_idx == 1 is
// ~A & ~C, == 2 is A & ~B (gc_frame_plot.py:7-28)
__device__ __forceinline__ ClsPre cls_counts(uint64_t A, uint64_t B, uint64_t C, uint64_t m) {
    uint64_t x0 = A & C, x1 = ~A & B;
    const uint64_t n0 = ~(A | C), n1 = A & ~B;
    x0 &= m; x1 &= m;
    ClsPre r;
    r.j00 = (uint32_t)__popcll(x0 & n0); r.j01 = (uint32_t)__popcll(x0 & n1); r.j10 = (uint32_t)__popcll(x1 & n0); r.j11 = (uint32_t)__popcll(x1 & n1);
    r.x0 = (uint32_t)__popcll(x0); r.x1 = (uint32_t)__popcll(x1); r.n0 = (uint32_t)__popcll(n0 & m); r.n1 = (uint32_t)__popcll(n1 & m);
    return r;
}
__device__ __forceinline__ void cls_add(ClsPre &a, const ClsPre &b) { a.j00 += b.j00; a.j01 += b.j01; a.j10 += b.j10; a.j11 += b.j11; a.x0 += b.x0; a.x1 += b.x1; a.n0 += b.n0; a.n1 += b.n1; }
__device__ __forceinline__ ClsPre cls_load(const ClsPre *p) { const uint4 u = ((const uint4 *)p)[0], v = ((const uint4 *)p)[1]; ClsPre r; r.j00 = u.x; r.j01 = u.y; r.j10 = u.z; r.j11 = u.w; r.x0 = v.x; r.x1 = v.y; r.n0 = v.z; r.n1 = v.w; return r; }

#define PRE_G PHX_PRE_G
__device__ __forceinline__ uint32_t wave_excl_scan_tot(uint32_t v, uint32_t *total) { // one wavefront, no barrier
    const uint32_t inc = wave_incl_scan(v);
    *total = (uint32_t)__shfl((int)inc, 63);
    return inc - v;
}
__device__ __forceinline__ void b_bit_prefix(const DBatch &b, const int bx, const int by, const int tx) { // one wavefront per (contig, plane): a lane takes PRE_G consecutive words
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0) return;
    const int nw = meta->nw; // a multiple of 8
    const uint64_t *bits = b.bits + meta->bits_off;
    const int64_t W = meta->bits_off / PHX_BITMAP_WORDS_PER_NW;
    const int plane = by; // 0..5: (strand, frame) class planes, 6: the base plane
    const int tid = tx;
    if (plane < 6) {
        const int fwd = plane < 3, f = plane % 3;
        const uint64_t *M = bits + (size_t)((fwd ? PHX_PLANE_GCF : PHX_PLANE_GCR) * 3 + f) * nw;
        const size_t st = (size_t)3 * nw;
        const int nrec = nw / PRE_G + 1;
        ClsPre *P = (ClsPre *)b.cpre + ((6 * W) / PRE_G + 6 * (int64_t)bx + plane * (int64_t)nrec);
        ClsPre carry = cls_counts(0, 0, 0, 0);
        for (int g0 = 0; g0 < nrec; g0 += 64) {
            const int g = g0 + tid, w0 = g * PRE_G;
            ClsPre loc = cls_counts(0, 0, 0, 0);
            if (w0 < nw)
#pragma unroll
                for (int k = 0; k < PRE_G; k++) cls_add(loc, cls_counts(M[w0 + k], M[st + w0 + k], M[2 * st + w0 + k], ~0ull));
            ClsPre ex, T;
            ex.j00 = wave_excl_scan_tot(loc.j00, &T.j00); ex.j01 = wave_excl_scan_tot(loc.j01, &T.j01);
            ex.j10 = wave_excl_scan_tot(loc.j10, &T.j10); ex.j11 = wave_excl_scan_tot(loc.j11, &T.j11);
            ex.x0 = wave_excl_scan_tot(loc.x0, &T.x0); ex.x1 = wave_excl_scan_tot(loc.x1, &T.x1);
            ex.n0 = wave_excl_scan_tot(loc.n0, &T.n0); ex.n1 = wave_excl_scan_tot(loc.n1, &T.n1);
            cls_add(ex, carry);
            if (g < nrec) { // record g: the counts over the words in front of group g (record nw / PRE_G: the totals)
                ((uint4 *)&P[g])[0] = make_uint4(ex.j00, ex.j01, ex.j10, ex.j11);
                ((uint4 *)&P[g])[1] = make_uint4(ex.x0, ex.x1, ex.n0, ex.n1);
            }
            cls_add(carry, T);
        }
    } else {
        // a lane takes `per` consecutive records; entry g = the counts in front of record g, entry 2 nw = the totals
        const uint32_t *__restrict__ rec = b.recs + (size_t)meta->rec_off * REC_WORDS;
        const int nrec = 2 * nw, per = (nrec + 63) / 64;
        uint4 *P = (uint4 *)b.bpre + (2 * W + 2 * (int64_t)bx);
        const int r0 = tid * per, r1 = r0 + per < nrec ? r0 + per : nrec;
        uint32_t la = 0, lc = 0, lt = 0, lg = 0;
        for (int r = r0; r < r1; r++) { uint32_t a, c, t, g; rec_counts(rec + (size_t)r * REC_WORDS, ~0u, ~0u, ~0u, a, c, t, g); la += a; lc += c; lt += t; lg += g; }
        uint32_t ta, tc, tt, tg;
        uint32_t ea = wave_excl_scan_tot(la, &ta), ec = wave_excl_scan_tot(lc, &tc), et = wave_excl_scan_tot(lt, &tt), eg = wave_excl_scan_tot(lg, &tg);
        for (int r = r0; r < r1; r++) { // (the records are in L1 / L2 from the first pass)
            P[r] = make_uint4(ea, ec, et, eg);
            uint32_t a, c, t, g; rec_counts(rec + (size_t)r * REC_WORDS, ~0u, ~0u, ~0u, a, c, t, g); ea += a; ec += c; et += t; eg += g;
        }
        if (tid == 63) P[nrec] = make_uint4(ta, tc, tt, tg);
        tail_windows(rec, meta->L, tid, meta->bg); // the 20 right-truncated forward background windows (functions.py:168), which k_features leaves out
    }
}
__global__ __launch_bounds__(64) void k_bit_prefix(DBatch b) { b_bit_prefix(b, (int)blockIdx.x, (int)blockIdx.y, (int)threadIdx.x); }


// 3x3 histogram (max_idx-1)*3 + (min_idx-1) over the codons [lo, hi] of one frame from the three comparison bitmaps M[0] = a > b,
// M[1] = b > c, M[2] = a > c of the strand (stride = distance between bitmaps; cls_counts): the words at the ends of the range
// are counted, the whole groups of PRE_G words between them come from the prefix records P of the plane
__device__ __forceinline__ void class_hist(const uint64_t *__restrict__ M, size_t stride, const ClsPre *__restrict__ P, int lo, int hi, uint32_t h[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] = 0;
    if (hi < lo) return;
    const int wl = lo >> 6, wh = hi >> 6;
    ClsPre c = cls_counts(0, 0, 0, 0);
    int a = (wl + PRE_G) & ~(PRE_G - 1), z = wh & ~(PRE_G - 1); // whole groups [a, z)
    if (z > a) {
        const ClsPre p1 = cls_load(P + z / PRE_G), p0 = cls_load(P + a / PRE_G);
        c.j00 = p1.j00 - p0.j00; c.j01 = p1.j01 - p0.j01; c.j10 = p1.j10 - p0.j10; c.j11 = p1.j11 - p0.j11;
        c.x0 = p1.x0 - p0.x0; c.x1 = p1.x1 - p0.x1; c.n0 = p1.n0 - p0.n0; c.n1 = p1.n1 - p0.n1;
    } else { a = wh + 1; z = wh + 1; }
    for (int w = wl; w <= wh; w++) {
        if (w == a) { w = z - 1; continue; }
        cls_add(c, cls_counts(M[w], M[stride + w], M[2 * stride + w], range_mask(w, lo, hi)));
    }
    const uint32_t N = (uint32_t)(hi - lo + 1);
    h[0] = c.j00; h[1] = c.j01; h[2] = c.x0 - c.j00 - c.j01;
    h[3] = c.j10; h[4] = c.j11; h[5] = c.x1 - c.j10 - c.j11;
    h[6] = c.n0 - c.j00 - c.j10; h[7] = c.n1 - c.j01 - c.j11;
    h[8] = N - c.x0 - c.x1 - c.n0 - c.n1 + c.j00 + c.j01 + c.j10 + c.j11;
}

// the sense codons of an ORF as a codon index range [clo, chi] of frame f on its strand's comparison planes: forward from the start to
// just before the stop / last codon (functions.py:290), reverse from just after the stop key up to the start codon (functions.py:295)
__device__ __forceinline__ void orf_codon_range(const DOrf &r, bool &fwd, int &f, int &clo, int &chi, int &lo1, int &hi1, int &ncod) {
    fwd = r.frame > 0;
    f = (fwd ? r.frame : -r.frame) - 1;
    // seq = positions [lo1, hi1] (1-based): fwd start..stop+2, rev stop..start+2 (functions.py:207,220)
    lo1 = fwd ? r.start : r.stop; hi1 = (fwd ? r.stop : r.start) + 2;
    ncod = (hi1 - lo1 + 1) / 3;
    const int k0 = (lo1 - 1 - f) / 3, k1 = k0 + ncod - 1;
    clo = fwd ? k0 : k0 + 1; chi = fwd ? k1 - 1 : k1;
}

// a, c, t, g counts over the 0-based positions [lo, hi] of a contig (rec: its records; bpre: its prefix entries, k_bit_prefix): the
// two records at the ends of the range are counted under per-stream masks, the records between them come from the prefix entries
__device__ __forceinline__ void base_counts(const uint32_t *__restrict__ rec, const uint4 *__restrict__ bpre, int lo, int hi, uint32_t &na, uint32_t &nc, uint32_t &nt, uint32_t &ng) {
    na = 0; nc = 0; nt = 0; ng = 0;
    if (hi < lo) return;
    const int wa = (lo / 3) >> 5, wb = (hi / 3) >> 5;
    uint32_t ma[3], mb[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int ka = lo > r ? (lo - r + 2) / 3 : 0;  // first index of stream r at or behind lo
        const int kb = hi >= r ? (hi - r) / 3 : -1;    // last index at or in front of hi
        const int sa = ka - 32 * wa, nb = kb - 32 * wb + 1;
        ma[r] = sa <= 0 ? ~0u : (sa >= 32 ? 0u : ~0u << sa);
        mb[r] = nb <= 0 ? 0u : (nb >= 32 ? ~0u : (1u << nb) - 1u);
    }
    if (wa == wb) { rec_counts(rec + (size_t)wa * REC_WORDS, ma[0] & mb[0], ma[1] & mb[1], ma[2] & mb[2], na, nc, nt, ng); return; }
    uint32_t a, c, t, g;
    rec_counts(rec + (size_t)wa * REC_WORDS, ma[0], ma[1], ma[2], na, nc, nt, ng);
    rec_counts(rec + (size_t)wb * REC_WORDS, mb[0], mb[1], mb[2], a, c, t, g);
    const uint4 p1 = bpre[wb], p0 = bpre[wa + 1];
    na += a + (p1.x - p0.x); nc += c + (p1.y - p0.y); nt += t + (p1.z - p0.z); ng += g + (p1.w - p0.w);
}

// What k_orf_stats needs of an ORF's start codon, from the 24 positions P0 .. P0 + 23 of the contig's bit planes (two consecutive
// records): forward ORF, start codon at q: the window dna[q - 20 : q + 1] read leftwards (functions.py:208-209; empty for q < 20) and
// the codon at q; reverse ORF, rc start codon at q .. q + 2: the codon and the window rev_comp(dna[q + 3 : q + 24]) (functions.py:221-222).
// Returns the score_rbs bin; ci = the codon's code (64: an ambiguous base in it).
__device__ __forceinline__ uint32_t spread3(uint32_t x) { // bit i of the low byte -> bit 3 i
    x = (x | (x << 8)) & 0x0000f00fu;
    x = (x | (x << 4)) & 0x000c30c3u;
    x = (x | (x << 2)) & 0x00249249u;
    return x;
}
__device__ __forceinline__ uint32_t start_window(const uint32_t *__restrict__ rec, bool fwd, int q, uint32_t &ci) {
    const int P0 = fwd ? (q >= 20 ? q - 20 : 0) : q;
    const int w0 = (P0 / 3) >> 5;
    const uint32_t *p = rec + (size_t)w0 * REC_WORDS;
    uint32_t lo[REC_WORDS], hi[REC_WORDS];
#pragma unroll
    for (int i = 0; i < REC_WORDS; i++) { lo[i] = p[i]; hi[i] = p[REC_WORDS + i]; } // (the record behind a contig's last one is its all-outside spacer)
    uint32_t lin[3] = {0, 0, 0}; // b0, b1, amb over the span: bit t <-> position P0 + t
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const int k = P0 > r ? (P0 - r + 2) / 3 : 0; // first index of stream r inside the span
        const int d = 3 * k + r - P0, sh = k - 32 * w0;
#pragma unroll
        for (int pl = 0; pl < 3; pl++) {
            const uint32_t f = (uint32_t)(((((uint64_t)hi[r * 3 + pl]) << 32) | lo[r * 3 + pl]) >> sh) & 0xffu;
            lin[pl] |= spread3(f) << d;
        }
    }
    const uint32_t ok = ~lin[2] & 0xffffffu;
    const uint32_t G = ok & lin[0] & lin[1], A = ok & ~lin[0] & ~lin[1], C = ok & lin[0] & ~lin[1], T = ok & ~lin[0] & lin[1];
    const int co = fwd ? q - P0 : 0;
    {
        const uint32_t a = (lin[2] >> co) & 7u;
        const uint32_t b0 = lin[0] >> co, b1 = lin[1] >> co;
        ci = a ? 64u : ((b0 & 1u) | ((b1 & 1u) << 1) | (((b0 >> 1) & 1u) << 2) | (((b1 >> 1) & 1u) << 3) | (((b0 >> 2) & 1u) << 4) | (((b1 >> 2) & 1u) << 5));
    }
    if (fwd) {
        if (q < 20) return 0u;
        // s[k] = dna[q - k] = span bit 20 - k
        const uint32_t Gs = __brev(G << 11), As = __brev(A << 11), nAs = __brev((C | T | G) << 11), nGs = __brev((A | C | T) << 11);
        return phxfc::rbs_bin_linear(Gs, As, nAs, nGs);
    }
    // s[k] = comp(dna[q + 3 + k]) = the complement of span bit 3 + k
    return phxfc::rbs_bin_linear(C >> 3, T >> 3, (A | C | G) >> 3, (A | T | G) >> 3);
}

__device__ __forceinline__ void b_orf_stats(const DBatch &b, const int bx, const int by, const int gy) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0) return;
    const DOrf *orf = b.orf + meta->orf_off;
    DOrfStat *ostat = b.ostat + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int nw = meta->nw;
    const uint32_t *__restrict__ rec = b.recs + (size_t)meta->rec_off * REC_WORDS;
    const uint64_t *bits = b.bits + meta->bits_off;
    const int64_t W = meta->bits_off / PHX_BITMAP_WORDS_PER_NW;
    const int npre = nw / PRE_G + 1;
    const ClsPre *cpre = (const ClsPre *)b.cpre + ((6 * W) / PRE_G + 6 * (int64_t)bx); // planes of nw / PRE_G + 1 records: forward frames 0..2, reverse frames 0..2
    const uint4 *bpre = (const uint4 *)b.bpre + (2 * W + 2 * (int64_t)bx);
    const DParams *__restrict__ P = b.params;
    const int gtid = (int)by * NT + (int)threadIdx.x, gstride = (int)gy * NT;
    __shared__ uint32_t s_tr[28]; // training_rbs of this workgroup's ORFs (one global atomic per bin instead of one per ORF)
    if (threadIdx.x < 28) s_tr[threadIdx.x] = 0;
    __syncthreads();
    for (int k = gtid; k < meta->n_orf; k += gstride) {
        const DOrf hd = orf[k]; // one 16-byte load
        const DOrf *r = &hd;
        const int start = r->start;
        const bool fwd = r->frame > 0;
        // what the ORF needs of its start codon, left out by k_orf<true>: the RBS bin of the window beside it (functions.py:208,221; from the
        // bases themselves: no per-position array), index of the start codon (-1 for a pseudo-start), Orf.start_codon() == 'atg'
        uint32_t bin, sidx, oflags;
        {
            uint32_t ci;
            bin = start_window(rec, fwd, start - 1, ci);
            const uint32_t at = P->atg_tab[ci]; // bit 0: 'atg', bit 1: 'cat' (= 'atg' on the reverse strand), bits 2..5: index of the start codon (of its reverse complement)
            const bool pseudo = (hd.flags >> 1) & 1u;
            sidx = pseudo ? 255u : (at >> 2);
            oflags = ((fwd ? at : at >> 1) & 1u) | (pseudo ? 2u : 0u);
        }
        bool fwd2; int f, clo, chi, lo1, hi1, ncod;
        orf_codon_range(hd, fwd2, f, clo, chi, lo1, hi1, ncod);
        // the record keeps the class counts in 16 bits: an ORF of more than 65535 codons (196 kb without an in-frame stop: an N run of
        // a scaffold) is marked and k_score counts its classes again, in 32 bits (the reference has no limit, functions.py:286-298)
        if (ncod > 65535) oflags |= 4u;
        uint32_t h[9];
        class_hist(bits + (size_t)((fwd ? PHX_PLANE_GCF : PHX_PLANE_GCR) * 3 + f) * nw, (size_t)3 * nw, cpre + (size_t)((fwd ? 0 : 3) + f) * npre, clo, chi, h);
        static_assert(sizeof(DOrfStat) == 32, "ORF statistics");
        uint32_t na, nc, nt, ng;
        base_counts(rec, bpre, lo1 - 1, hi1 - 1, na, nc, nt, ng);
        if (!fwd) { const uint32_t t = na; na = nt; nt = t; ng = nc; } // coding strand: a<->t, g<->c
        // Orf.p_stop, orfs.py:162-173
        const double n = (double)(3 * ncod);
        const double Pa = (double)na / n, Pt = (double)nt / n, Pg = (double)ng / n;
        const double pstop = Pt * Pa * Pa + Pt * Pg * Pa + Pt * Pa * Pg;
        uint4 *sp = (uint4 *)&ostat[k]; // the whole record as two 16-byte stores
        if (oflags & 4u) for (int i = 0; i < 9; i++) h[i] = h[i] > 65535u ? 65535u : h[i];
        sp[0] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
        sp[1] = make_uint4(h[8] | (bin << 16) | (sidx << 24), oflags, (uint32_t)__double_as_longlong(pstop), (uint32_t)((unsigned long long)__double_as_longlong(pstop) >> 32));
        atomicAdd(&s_tr[bin], 1u); // training_rbs, functions.py:211,224,239,251
    }
    __syncthreads();
    if (threadIdx.x < 28 && s_tr[threadIdx.x]) atomicAdd(&meta->tr[threadIdx.x], s_tr[threadIdx.x]);
    // GC frame plot training: per group, the first ORF longest->shortest whose start codon is 'atg'
    for (int g = gtid; g < meta->n_grp; g += gstride) {
        const DGrp G = grp[g];
        const int pick = G.pick; // emission order is nearest-first, iter_in is farthest-first (orfs.py:38-46): the last 'atg' ORF emitted
        if (pick < 0) continue;
        const DOrf *r = &orf[G.orf_begin + pick];
        const int start = r->start, stop = r->stop;
        const bool fwd = start < stop;
        const int f = (start - 1) % 3;
        int clo, chi; // codon index range (inclusive) of the bases visited by the training loop
        if (fwd) { // range(start+n, stop-36, 3), functions.py:270-271
            const int nn = (int)((double)(stop - start) / 8.0) * 3;
            clo = (start + nn - 1 - f) / 3;
            chi = (stop - 36 - 1 - 1 - f) / 3; // last base < stop-36 in this frame
            if (stop - 36 - 1 - 1 - f < 0) chi = -1;
        } else if (stop < start) { // range(start-n, stop+36, -3), functions.py:275-276
            const int nn = (int)((double)(start - stop) / 8.0) * 3;
            chi = (start - nn - 1 - f) / 3;
            clo = (stop + 36 - 1 - f) / 3 + 1; // first base > stop+36 in this frame
        } else continue;
        uint32_t mx[3] = {0, 0, 0}, mn[3] = {0, 0, 0};
        {
            uint32_t h[9];
            class_hist(bits + (size_t)((fwd ? PHX_PLANE_GCF : PHX_PLANE_GCR) * 3 + f) * nw, (size_t)3 * nw, cpre + (size_t)((fwd ? 0 : 3) + f) * npre, clo, chi, h);
            for (int cl = 0; cl < 9; cl++) { mx[cl / 3] += h[cl]; mn[cl % 3] += h[cl]; }
        }
        for (int i = 0; i < 3; i++) {
            if (mx[i]) atomicAdd(&meta->pmax[i + 1], mx[i]);
            if (mn[i]) atomicAdd(&meta->pmin[i + 1], mn[i]);
        }
    }
}
__global__ __launch_bounds__(NT) void k_orf_stats(DBatch b) { b_orf_stats(b, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y); }


// ORF weight: functions.py:254-257 (RBS), 281-284 (normalise), 286-301 + orfs.py:122-127.
// hold = prod ((1-pstop)^pos_max[imax])^pos_min[imin] = (1-pstop)^S ; weight = -(1/hold)*w_start*w_rbs
__device__ __forceinline__ void b_score(const DBatch &b, const int bx) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    __shared__ int s_maxexp;
    __shared__ double s_wsum;
    DMeta *meta = &b.meta[bx];
    if (meta->status < 0) return;
    if (threadIdx.x == 0) { s_maxexp = 0; s_wsum = 0.0; }
    __syncthreads();
    const DOrfStat *ostat = b.ostat + meta->orf_off;
    double *oweight = b.oweight + meta->orf_off;
    long long *owi = b.owi + meta->orf_off;
    uint8_t *oflag = b.oflag + meta->orf_off;
    const double cc = CERT_C(b);
    const DParams *P = b.params;
    double bgs = 0, trs = 0;
    for (int i = 0; i < 28; i++) { bgs += 1.0 + (double)meta->bg[i]; trs += 1.0 + (double)meta->tr[i]; }
    double pmax[4], pmin[4];
    {
        double ymx = 1.0, ymn = 1.0;
        for (int i = 0; i < 4; i++) {
            pmax[i] = 1.0 + (double)(i ? meta->pmax[i] : 0u);
            pmin[i] = 1.0 + (double)(i ? meta->pmin[i] : 0u);
            ymx = pmax[i] > ymx ? pmax[i] : ymx;
            ymn = pmin[i] > ymn ? pmin[i] : ymn;
        }
        for (int i = 0; i < 4; i++) { pmax[i] /= ymx; pmin[i] /= ymn; }
    }
    int mymax = 0;
    double mysum = 0.0;
    for (int k = threadIdx.x; k < meta->n_orf; k += (int)blockDim.x) { // (NT threads; one wavefront for batches of short contigs)
        const DOrfStat st = ostat[k];
        uint32_t h[9];
        for (int i = 0; i < 9; i++) h[i] = st.hist[i];
        if (st.flags & 4u) { // more than 65535 codons: the record's counts are clipped, counted again here (k_orf_stats)
            const DOrf hd = b.orf[meta->orf_off + k];
            bool fwd; int f, clo, chi, lo1, hi1, ncod;
            orf_codon_range(hd, fwd, f, clo, chi, lo1, hi1, ncod);
            const int nw = meta->nw, npre = nw / PRE_G + 1;
            const int64_t W = meta->bits_off / PHX_BITMAP_WORDS_PER_NW;
            const ClsPre *cpre = (const ClsPre *)b.cpre + ((6 * W) / PRE_G + 6 * (int64_t)bx);
            class_hist(b.bits + meta->bits_off + (size_t)((fwd ? PHX_PLANE_GCF : PHX_PLANE_GCR) * 3 + f) * nw, (size_t)3 * nw, cpre + (size_t)((fwd ? 0 : 3) + f) * npre, clo, chi, h);
        }
        double S = 0;
        for (int a = 0; a < 3; a++)
            for (int c = 0; c < 3; c++) S += (double)h[a * 3 + c] * (pmax[a + 1] * pmin[c + 1]);
        const double tr = (1.0 + (double)meta->tr[st.rbs]) / trs;
        const double bg = (1.0 + (double)meta->bg[st.rbs]) / bgs;
        const double w_rbs = tr / bg;
        double s = exp(-S * log1p(-st.pstop));
        if (st.startidx >= 0) s = s * P->start_w[st.startidx];
        s = s * w_rbs;
        const double w = s != 0.0 ? -s : 0.0; // weight = -s; Decimal's minus of a zero is +0 (a start weight of 0): "0.000000E+00", not "-0..."
        oweight[k] = w;
        owi[k] = ew_encode(w); // what the solver adds (edges.py:22), and whether the reference's integer may differ from it (k_certify)
        oflag[k] = (uint8_t)((cert_eps_is_zero_fast(w, cc) ? 0 : 2) | (ew_narrow51(owi[k]) ? 0 : 1));
        int e;
        frexp(s * 1000.0, &e);
        if (!(s < 1.0e300)) e = 4096; // inf / nan: force the overflow status
        mymax = e > mymax ? e : mymax;
        if (s < 1.0e300) mysum += s * 1000.0;
    }
    if (mymax) { atomicMax(&s_maxexp, mymax); atomicAdd(&s_wsum, mysum); }
    __syncthreads();
    if (threadIdx.x == 0) { meta->maxexp = s_maxexp; meta->wsum = s_wsum; }
}
__global__ __launch_bounds__(NT) void k_score(DBatch b) { b_score(b, (int)blockIdx.x); }
// a few long contigs (T4 alone: ~6000 ORFs on 256 threads took 32 us): the same body on 1024 threads
__global__ __launch_bounds__(1024) void k_score_big(DBatch b) { b_score(b, (int)blockIdx.x); }


