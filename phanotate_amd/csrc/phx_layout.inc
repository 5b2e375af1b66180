// phx_layout.inc — k_layout1 / k_layout2: batch layout on the device (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// Batch layout on the device.  One workgroup walks the contigs (a scan per 1024), so that no host round trip is
// needed between the counting and the emitting kernels when the buffers of the context are large enough.
#define LAYOUT_T 1024
#define LAYOUT_PER 16
// four running sums at once
__device__ __forceinline__ void layout_scan4(int64_t v[4], int64_t base[4], int64_t *s_part /* [4][LAYOUT_T/64 + 1] */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t inc[4];
    for (int q = 0; q < 4; q++) {
        int64_t x = v[q];
        for (int d = 1; d < 64; d <<= 1) { const int64_t t = __shfl_up(x, d); if (lane >= d) x += t; }
        inc[q] = x;
        if (lane == 63) s_part[q * 17 + w] = x;
    }
    __syncthreads();
    if (threadIdx.x < 4) { int64_t a = 0; for (int i = 0; i < LAYOUT_T / 64; i++) { const int64_t t = s_part[threadIdx.x * 17 + i]; s_part[threadIdx.x * 17 + i] = a; a += t; } s_part[threadIdx.x * 17 + 16] = a; }
    __syncthreads();
    for (int q = 0; q < 4; q++) { const int64_t ex = base[q] + s_part[q * 17 + w] + inc[q] - v[q]; const int64_t tot = s_part[q * 17 + 16]; v[q] = ex; inc[q] = tot; }
    __syncthreads();
    for (int q = 0; q < 4; q++) base[q] += inc[q];
}
// after k_orf<false>: ORF / group / node / close-bitmap offsets (what phx_run did on the host between two syncs)
__global__ __launch_bounds__(LAYOUT_T) void k_layout1(DBatch b) {
    __shared__ int64_t s_part[4 * 17];
    int64_t base[4] = {0, 0, 0, 0};
    // a thread takes `per` consecutive contigs per round (1 for batches of up to 1024 contigs, up to LAYOUT_PER for large batches of
    // short contigs, where a round per 1024 contigs made this single workgroup a bottleneck)
    const int per = b.n_contig <= LAYOUT_T ? 1 : (b.n_contig + LAYOUT_T - 1) / LAYOUT_T < LAYOUT_PER ? (b.n_contig + LAYOUT_T - 1) / LAYOUT_T : LAYOUT_PER;
    for (int i0 = 0; i0 < b.n_contig; i0 += LAYOUT_T * per) {
        const int ia = i0 + (int)threadIdx.x * per;
        int64_t v[4] = {0, 0, 0, 0};
        for (int k = 0; k < per && ia + k < b.n_contig; k++) {
            DMeta *m = &b.meta[ia + k];
            const int n_node = m->status < 0 ? 0 : m->n_orf + m->n_grp + (b.tnode ? m->n_tnode : 0) + 2;
            v[0] += m->n_orf; v[1] += m->n_grp; v[2] += n_node; v[3] += 2 * (int64_t)(n_node / 64 + 1);
        }
        layout_scan4(v, base, s_part);
        for (int k = 0; k < per && ia + k < b.n_contig; k++) {
            DMeta *m = &b.meta[ia + k];
            const int n_node = m->status < 0 ? 0 : m->n_orf + m->n_grp + (b.tnode ? m->n_tnode : 0) + 2;
            const int ncw = n_node / 64 + 1;
            m->orf_off = v[0]; m->grp_off = v[1]; m->node_off = v[2]; m->cb_off = v[3];
            m->n_node = n_node; m->ncw = ncw;
            // window records of k_sssp_wave: room for n_node/16 + 7 per contig without a scan of its own
            m->win_off = v[2] / 16 + 8 * (int64_t)(ia + k); m->n_win = 0;
            v[0] += m->n_orf; v[1] += m->n_grp; v[2] += n_node; v[3] += 2 * (int64_t)ncw;
        }
    }
    if (threadIdx.x == 0) {
        DTotals *t = b.tot;
        t->orf = base[0]; t->grp = base[1]; t->node = base[2]; t->cb = base[3];
        if (base[0] > b.caps.orf || base[1] > b.caps.grp || base[2] > b.caps.node || base[3] > b.caps.cb || base[2] / 16 + 8 * (int64_t)b.n_contig + 8 > b.caps.win) { if (!(b.caps.flags & 4)) t->overflow |= 1; }
    }
}


// ------------------------------------------------------------------------------------------------
// The same for batches of many (short) contigs: one workgroup for 20 000 contigs took 0.2 / 0.4 ms.  Pass A: a workgroup per LMB_T
// contigs, a thread per contig: its counts, offsets relative to the workgroup, the workgroup's totals to DBatch.lpart.  Pass B: every
// workgroup adds the totals of the ones in front of it to its contigs; the last one writes the batch totals.
#define LMB_T 256
__device__ __forceinline__ void lmb_scan4(int64_t v[4], int64_t tot[4], int64_t *s_part /* [4][LMB_T/64 + 1] */) { // exclusive scan over the workgroup, v in place
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t inc[4];
    for (int q = 0; q < 4; q++) {
        int64_t x = v[q];
        for (int d = 1; d < 64; d <<= 1) { const int64_t t = __shfl_up(x, d); if (lane >= d) x += t; }
        inc[q] = x;
        if (lane == 63) s_part[q * 5 + w] = x;
    }
    __syncthreads();
    if (threadIdx.x < 4) { int64_t a = 0; for (int i = 0; i < LMB_T / 64; i++) { const int64_t t = s_part[threadIdx.x * 5 + i]; s_part[threadIdx.x * 5 + i] = a; a += t; } s_part[threadIdx.x * 5 + 4] = a; }
    __syncthreads();
    for (int q = 0; q < 4; q++) { v[q] = s_part[q * 5 + w] + inc[q] - v[q]; tot[q] = s_part[q * 5 + 4]; }
    __syncthreads();
}
// sum of the totals of the workgroups in front of this one
__device__ __forceinline__ void lmb_base(const int64_t *lpart, int64_t base[4], int64_t *s_part, const int bx) {
    int64_t a[4] = {0, 0, 0, 0};
    for (int j = threadIdx.x; j < bx; j += LMB_T)
        for (int q = 0; q < 4; q++) a[q] += lpart[(size_t)j * 4 + q];
    for (int q = 0; q < 4; q++) {
        int64_t x = a[q];
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d);
        if ((threadIdx.x & 63) == 0) s_part[q * 5 + (threadIdx.x >> 6)] = x;
    }
    __syncthreads();
    for (int q = 0; q < 4; q++) { base[q] = 0; for (int i = 0; i < LMB_T / 64; i++) base[q] += s_part[q * 5 + i]; }
    __syncthreads();
}
__device__ __forceinline__ void b_layout1_a(const DBatch &b, const int bx, const int gx) {
    __shared__ int64_t s_part[4 * 5];
    const int i = (int)bx * LMB_T + (int)threadIdx.x;
    int64_t v[4] = {0, 0, 0, 0}, tot[4];
    int n_node = 0;
    if (i < b.n_contig) {
        DMeta *m = &b.meta[i];
        n_node = m->status < 0 ? 0 : m->n_orf + m->n_grp + (b.tnode ? m->n_tnode : 0) + 2;
        v[0] = m->n_orf; v[1] = m->n_grp; v[2] = n_node; v[3] = 2 * (int64_t)(n_node / 64 + 1);
    }
    lmb_scan4(v, tot, s_part);
    if (i < b.n_contig) {
        DMeta *m = &b.meta[i];
        m->orf_off = v[0]; m->grp_off = v[1]; m->node_off = v[2]; m->cb_off = v[3]; // relative to the workgroup: k_layout1_b adds its base
        m->n_node = n_node; m->ncw = n_node / 64 + 1; m->n_win = 0;
    }
    if (threadIdx.x < 4) b.lpart[(size_t)bx * 4 + threadIdx.x] = tot[threadIdx.x];
}
__global__ __launch_bounds__(LMB_T) void k_layout1_a(DBatch b) { b_layout1_a(b, (int)blockIdx.x, (int)gridDim.x); }

__device__ __forceinline__ void b_layout1_b(const DBatch &b, const int bx, const int gx) {
    __shared__ int64_t s_part[4 * 5];
    int64_t base[4];
    lmb_base(b.lpart, base, s_part, bx);
    const int i = (int)bx * LMB_T + (int)threadIdx.x;
    if (i < b.n_contig) {
        DMeta *m = &b.meta[i];
        m->orf_off += base[0]; m->grp_off += base[1]; m->node_off += base[2]; m->cb_off += base[3];
        m->win_off = m->node_off / 16 + 8 * (int64_t)i; // window records of k_sssp_wave: room for n_node/16 + 7 per contig without a scan of its own
    }
    if (bx == gx - 1 && threadIdx.x == 0) {
        DTotals *t = b.tot;
        for (int q = 0; q < 4; q++) base[q] += b.lpart[(size_t)bx * 4 + q];
        t->orf = base[0]; t->grp = base[1]; t->node = base[2]; t->cb = base[3];
        if (base[0] > b.caps.orf || base[1] > b.caps.grp || base[2] > b.caps.node || base[3] > b.caps.cb || base[2] / 16 + 8 * (int64_t)b.n_contig + 8 > b.caps.win) { if (!(b.caps.flags & 4)) t->overflow |= 1; }
    }
}
__global__ __launch_bounds__(LMB_T) void k_layout1_b(DBatch b) { b_layout1_b(b, (int)blockIdx.x, (int)gridDim.x); }



// Bits the path sums of one contig need.  A tentative distance is the length of a walk that uses every ORF edge at most once (a shortest
// path is simple; longer walks never win), so |dist| <= B = sum |w_orf| + (V/2) * max |w_connector| + extra.  The connector bound follows
// functions.py:26-46: overlap < 500 bp, gap <= 300 bp or bridge pow(.)+length; terminals are smaller still.  A candidate d(u)+w needs one
// more bit, the sign another, the "unreached" pattern sits two bits higher; one bit covers the rounding of the fp64 sum.
// extra: 0 for the layout; the evidence-weighted re-annotation (phx_resolve.inc, DESIGN.md §19) passes the sum of |B| over the contig's
// biased edges — each is used at most once as well.
__device__ __forceinline__ int contig_sum_bits(const DBatch &b, const DMeta *m, double extra) {
    if (m->maxexp >= 2000) return 4096;
    const double pst = contig_pstop(m->gc, m->L);
    double cmax = 1.0 / pow(1.0 - pst, 500.0);
    const double c2 = 1.0 / pow(1.0 - pst, 100.0);
    cmax = (cmax > c2 ? cmax : c2) + 20.0;
    const double c3 = (double)m->L + 21.0;
    cmax = (cmax > c3 ? cmax : c3) * 1000.0;
    double bound = m->wsum + 20000.0 * (double)(b.tnode ? m->n_tedge : 0) + 0.5 * (double)(m->n_node > 2 ? m->n_node : 2) * cmax;
    if (extra > 0.0) bound += extra;
    int eb = 0;
    (void)frexp(bound, &eb);
    return (eb > m->maxexp ? eb : m->maxexp) + 5;
}

// integer class and solver of one contig (accumulators of the workgroup: widest class, kernel mask, largest node count, LDS needs);
// returns its edge count
__device__ __forceinline__ int64_t layout2_contig(const DBatch &b, DMeta *m, bool force_global, bool no_wave, int *s_nl, int *s_mask, int *s_vmax, unsigned long long *s_lds) {
    int64_t ne = 0;
        m->sssp_nl = 2; m->sssp_mode = 0; m->sssp_fb = 0;
        if (m->status < 0) m->n_edge = 0;
        else {
            ne = m->n_edge;
            const int bits = contig_sum_bits(b, m, 0.0);
            if (bits > 17 * 64) {
                // beyond the widest integer kernel (an ORF weight beyond ~1e300: fp64 itself gives up): no device kernel solves this contig.
                // Its graph is still built — nodes, edge rows, flags —, k_results reports PHX_S_OVERFLOW, and phx_download* solve it on
                // the host in the reference's own arithmetic, which has no limit (CHANGELOG.md:11-13; phx_exact.inc), unless exactness is off
                m->sssp_nl = 0; m->sssp_mode = 4; m->sssp_fb = 4; m->cert = 0;
            } else {
                const int k = bits <= 128 ? 0 : bits <= 256 ? 1 : bits <= 512 ? 2 : 3;
                const int nl = k == 0 ? 2 : k == 1 ? 4 : k == 2 ? 8 : 17;
                m->sssp_nl = nl;
                const size_t lds = sssp_lds_bytes(m->n_node, nl);
                // the kernel a contig falls back to when the wavefront kernel hands it back (and the one it gets otherwise)
                const int fb = force_global ? 0 : (lds <= 158 * 1024 ? 1 : 0);
                const int mode = (!force_global && !no_wave && (nl == 2 || nl == 4 || nl == 8) && !(m->dense & 1)) ? 2 : fb; // dense: its windows would not fit, see k_edges
                m->sssp_fb = fb; m->sssp_mode = mode;
                atomicMax(s_nl, nl);
                if (m->n_node <= 2) m->cert = 1; // no graph: nothing to certify, and no k_certify launch may ever see this contig's limb class
                if (m->n_node > 2) {
                    atomicOr(s_mask, (1 << (4 * k + mode)) | (mode == 2 ? 1 << (4 * k + fb) : 0) | (((m->dense & 1) && mode == 1) ? 1 << (16 + k) : 0));
                    if (fb == 1) atomicMax(&s_lds[k], (unsigned long long)lds);
                    atomicMax(s_vmax, m->n_node);
                }
            }
        }
    return ne;
}

// after k_edges<false>: edge offsets; per contig the integer width its path sums need and the kernel that solves it
__global__ __launch_bounds__(LAYOUT_T) void k_layout2(DBatch b) {
    __shared__ int64_t s_part[4 * 17];
    __shared__ int s_nl, s_mask, s_vmax;
    __shared__ unsigned long long s_lds[4];
    if (b.tot->overflow) return;
    if (threadIdx.x == 0) { s_nl = 2; s_mask = 0; s_vmax = 0; for (int k = 0; k < 4; k++) s_lds[k] = 0; }
    __syncthreads();
    int64_t base[4] = {0, 0, 0, 0};
    const bool force_global = b.caps.flags & 1, no_wave = (b.caps.flags & 2) != 0;
    auto per_contig = [&](DMeta *m) -> int64_t { return layout2_contig(b, m, force_global, no_wave, &s_nl, &s_mask, &s_vmax, s_lds); };
    const int per = b.n_contig <= LAYOUT_T ? 1 : (b.n_contig + LAYOUT_T - 1) / LAYOUT_T < LAYOUT_PER ? (b.n_contig + LAYOUT_T - 1) / LAYOUT_T : LAYOUT_PER;
    for (int i0 = 0; i0 < b.n_contig; i0 += LAYOUT_T * per) {
        const int ia = i0 + (int)threadIdx.x * per;
        int64_t v[4] = {0, 0, 0, 0};
        int64_t mine[LAYOUT_PER];
        for (int k = 0; k < per && ia + k < b.n_contig; k++) { mine[k] = per_contig(&b.meta[ia + k]); v[0] += mine[k]; }
        layout_scan4(v, base, s_part);
        for (int k = 0; k < per && ia + k < b.n_contig; k++) { b.meta[ia + k].edge_off = v[0]; v[0] += mine[k]; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        DTotals *t = b.tot;
        t->edge = base[0]; t->nlmax = s_nl; t->class_mask = s_mask; t->vmax = s_vmax;
        for (int k = 0; k < 4; k++) t->lds_need[k] = (int64_t)s_lds[k];
        if ((base[0] + 1 > b.caps.edge || s_nl > b.caps.limbs) && !(b.caps.flags & 4)) t->overflow |= 2;
    }
}

// multi-workgroup form for large batches (see k_layout1_a / _b)
__device__ __forceinline__ void b_layout2_a(const DBatch &b, const int bx, const int gx) {
    __shared__ int64_t s_part[4 * 5];
    __shared__ int s_nl, s_mask, s_vmax;
    __shared__ unsigned long long s_lds[4];
    if (b.tot->overflow) return;
    if (threadIdx.x == 0) { s_nl = 2; s_mask = 0; s_vmax = 0; for (int k = 0; k < 4; k++) s_lds[k] = 0; }
    __syncthreads();
    const bool force_global = b.caps.flags & 1, no_wave = (b.caps.flags & 2) != 0;
    const int i = (int)bx * LMB_T + (int)threadIdx.x;
    int64_t v[4] = {0, 0, 0, 0}, tot[4];
    if (i < b.n_contig) v[0] = layout2_contig(b, &b.meta[i], force_global, no_wave, &s_nl, &s_mask, &s_vmax, s_lds);
    lmb_scan4(v, tot, s_part);
    if (i < b.n_contig) b.meta[i].edge_off = v[0]; // relative to the workgroup: k_layout2_b adds its base
    if (threadIdx.x < 4) b.lpart[(size_t)bx * 4 + threadIdx.x] = tot[threadIdx.x];
    if (threadIdx.x == 0) {
        DTotals *t = b.tot;
        atomicMax(&t->nlmax, s_nl); atomicOr(&t->class_mask, s_mask); atomicMax(&t->vmax, s_vmax);
        for (int k = 0; k < 4; k++) if (s_lds[k]) atomicMax((unsigned long long *)&t->lds_need[k], s_lds[k]);
    }
}
__global__ __launch_bounds__(LMB_T) void k_layout2_a(DBatch b) { b_layout2_a(b, (int)blockIdx.x, (int)gridDim.x); }

__device__ __forceinline__ void b_layout2_b(const DBatch &b, const int bx, const int gx) {
    __shared__ int64_t s_part[4 * 5];
    if (b.tot->overflow) return;
    int64_t base[4];
    lmb_base(b.lpart, base, s_part, bx);
    const int i = (int)bx * LMB_T + (int)threadIdx.x;
    if (i < b.n_contig) b.meta[i].edge_off += base[0];
    if (bx == gx - 1 && threadIdx.x == 0) {
        DTotals *t = b.tot;
        t->edge = base[0] + b.lpart[(size_t)bx * 4];
        if ((t->edge + 1 > b.caps.edge || t->nlmax > b.caps.limbs) && !(b.caps.flags & 4)) t->overflow |= 2;
    }
}
__global__ __launch_bounds__(LMB_T) void k_layout2_b(DBatch b) { b_layout2_b(b, (int)blockIdx.x, (int)gridDim.x); }


// Gene records of a batch of many contigs (DBatch.gpack): every contig wrote its genes at its own place (one shared counter for 20 000
// small contigs was 0.25 ms of same-address atomics); here they move together, in contig order.  Pass A: gene count per workgroup of 256
// contigs; pass B: offsets, then the workgroup copies its records, one record per thread and step.
__global__ __launch_bounds__(LMB_T) void k_gene_pack_a(DBatch b) {
    __shared__ int64_t s_part[4 * 5];
    const int i = (int)blockIdx.x * LMB_T + (int)threadIdx.x;
    int64_t v[4] = {0, 0, 0, 0}, tot[4];
    if (i < b.n_contig && b.meta[i].status >= 0) v[0] = b.meta[i].n_genes;
    lmb_scan4(v, tot, s_part);
    if (threadIdx.x < 4) b.lpart[(size_t)blockIdx.x * 4 + threadIdx.x] = tot[threadIdx.x];
}
__global__ __launch_bounds__(LMB_T) void k_gene_pack_b(DBatch b) {
    __shared__ int64_t s_part[4 * 5];
    __shared__ uint32_t s_dst[LMB_T + 1]; // workgroup-relative first record of every contig (+ the total)
    __shared__ int64_t s_src[LMB_T];
    int64_t base[4];
    lmb_base(b.lpart, base, s_part, (int)blockIdx.x);
    const int i = (int)blockIdx.x * LMB_T + (int)threadIdx.x;
    int64_t v[4] = {0, 0, 0, 0}, tot[4];
    int64_t src = 0;
    if (i < b.n_contig && b.meta[i].status >= 0) { v[0] = b.meta[i].n_genes; src = b.meta[i].grp_off + b.meta[i].tn_off; } // the contig's own place (not gene_off: the first workgroup of the row rewrites that)
    lmb_scan4(v, tot, s_part);
    s_dst[threadIdx.x] = (uint32_t)v[0];
    s_src[threadIdx.x] = src;
    if (threadIdx.x == 0) s_dst[LMB_T] = (uint32_t)tot[0];
    __syncthreads();
    if (i < b.n_contig && blockIdx.y == 0) b.meta[i].gene_off = base[0] + v[0];
    const uint64_t *from = (const uint64_t *)b.genes;
    uint64_t *to = (uint64_t *)(b.genes_c + base[0]);
    static_assert(sizeof(DGene) == 24, "gene record");
    for (uint32_t f = threadIdx.x + blockIdx.y * LMB_T; f < s_dst[LMB_T]; f += LMB_T * gridDim.y) { // gridDim.y workgroups share the records of 256 contigs
        int lo = 0, hi = LMB_T; // the contig of record f: the last one with s_dst <= f
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_dst[mid] <= f) lo = mid; else hi = mid; }
        const uint64_t *p = from + (size_t)(s_src[lo] + (f - s_dst[lo])) * 3;
        const uint64_t x0 = p[0], x1 = p[1], x2 = p[2];
        uint64_t *q = to + (size_t)f * 3;
        q[0] = x0; q[1] = x1; q[2] = x2;
    }
}

// the last kernel of a run: what the host reads of every contig (16 bytes instead of the whole record)
__global__ __launch_bounds__(LMB_T) void k_results(DBatch b) {
    const int i = (int)blockIdx.x * LMB_T + (int)threadIdx.x;
    if (i >= b.n_contig) return;
    if (i == 0) *(DTotals *)(b.res + b.n_contig) = *b.tot; // final by now; behind the records, so that one copy takes both to the host
    const DMeta *m = &b.meta[i];
    DRes r;
    r.status = (m->status == 0 && m->sssp_mode == 4 && m->n_node > 2) ? PHX_S_OVERFLOW : m->status; // (mode 4: the host's to solve, see k_layout2)
    r.n_genes = m->n_genes; r.gene_off = m->gene_off; r.cert = m->cert; r.tie = m->tie;
    b.res[i] = r;
}

// The head of a run in one launch (it was three fills and a copy: four graph nodes of ~5 us each): node / coverage bitmaps and the tRNA
// node bitmaps to zero, the totals and the gene counter to zero, the per-contig records back to what the layout set (accumulators zero).
__global__ __launch_bounds__(256) void k_reset(DBatch b, const DMeta *__restrict__ meta0, unsigned long long nbits_words, unsigned long long tbits_words) {
    const size_t gt = (size_t)blockIdx.x * 256 + threadIdx.x, gs = (size_t)gridDim.x * 256;
    const uint4 z = make_uint4(0, 0, 0, 0);
    for (size_t i = gt; 2 * i < nbits_words; i += gs) ((uint4 *)b.nbits)[i] = z;      // (the buffers end in slack: a pair may run one word over)
    if (b.tbits) for (size_t i = gt; 2 * i < tbits_words; i += gs) ((uint4 *)b.tbits)[i] = z;
    static_assert(sizeof(DMeta) % 8 == 0 && sizeof(DTotals) % 8 == 0, "copied as 64-bit words");
    const size_t mw = (size_t)b.n_contig * (sizeof(DMeta) / 8);
    for (size_t i = gt; i < mw; i += gs) ((uint64_t *)b.meta)[i] = ((const uint64_t *)meta0)[i];
    if (gt < sizeof(DTotals) / 8) ((uint64_t *)b.tot)[gt] = 0ull;
    if (gt < 8) ((uint64_t *)b.gene_total)[gt] = 0ull; // 64 bytes
    if (b.segw) for (size_t i = gt; i < (size_t)b.segw_ints; i += gs) b.segw[i] = 0; // (segments: a solver that follows its planner reads "no window yet")
}

// Launch order of k_sssp_wave for batches with more contigs than SIMDs (one wavefront of that kernel per SIMD): the workgroups
// beyond the first round start as earlier ones finish, so the contigs with the most in-edges go first and the second round is
// left with the short ones (windows or nodes as the key do as well as in-edges).  A counting sort on 256 levels of n_edge by one workgroup (order inside a level: as the atomics fall;
// it only decides when a contig is solved, not what comes out).
__global__ __launch_bounds__(LMB_T) void k_sssp_order(DBatch b) {
    __shared__ uint32_t s_max, s_cnt[256], s_scan[LMB_T / 64 + 1];
    const int tid = threadIdx.x, n = b.n_contig;
    if (b.tot->overflow) return;
    if (tid == 0) s_max = 1;
    static_assert(LMB_T == 256, "k_sssp_order: one thread per level");
    s_cnt[tid] = 0;
    __syncthreads();
    uint32_t mx = 0;
    for (int i = tid; i < n; i += LMB_T) { const DMeta *m = &b.meta[i]; const uint32_t e = m->status < 0 ? 0u : (uint32_t)m->n_edge; mx = e > mx ? e : mx; }
    atomicMax(&s_max, mx);
    __syncthreads();
    const uint64_t top = s_max;
    auto level = [&](int i) { const DMeta *m = &b.meta[i]; const uint64_t e = m->status < 0 ? 0u : (uint32_t)m->n_edge; return 255u - (uint32_t)(e * 255u / top); };
    for (int i = tid; i < n; i += LMB_T) atomicAdd(&s_cnt[level(i)], 1u);
    __syncthreads();
    uint32_t tot;
    const uint32_t mine = s_cnt[tid], ex = block_excl_scan<LMB_T>(mine, s_scan, &tot);
    __syncthreads();
    s_cnt[tid] = ex;
    __syncthreads();
    for (int i = tid; i < n; i += LMB_T) b.sord[atomicAdd(&s_cnt[level(i)], 1u)] = i;
}
