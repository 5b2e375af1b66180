// phx_resolve.inc — masked re-annotation: the best path without a chosen set of ORFs (included by phx_kernels.hip; DESIGN.md §14).
// ------------------------------------------------------------------------------------------------
// On demand after a run, kernel by kernel on the context's stream; never in phx_run, the captured graph or the certificate path.
// The kernels get TWO views of the batch: the graph (in_off / esrc / ew / gtab, nodes, ORFs, groups) is the run's, read only; every output
// (DMeta, DTotals, dist, parent, path, genes, gene_total, the tie scratch) is the re-annotation's own — the DBatch they receive is the run's with
// those pointers replaced (phx_api.cpp, reann_batch), so the device code shared with the run (inorder_contig, emit_genes) writes nothing the
// run's results live in.
//
//   k_rs_mask      a thread per ORF: a refused ORF finds its edge (as k_margins does: among the in-edges of its right node, by its source)
//                  and sets that in-edge slot's bit.  One bit per in-edge slot of the batch, cleared per call.
//   k_rs_lds<NL>   lds_sweep (phx_sssp.inc), the windowed workgroup-per-contig sweep of k_sssp_lds, under the MASKED policy RsCfg<NL>: over
//                  G_F, on the rows as the graph stage left them (no k_edges_expand).  What MASKED means is said at the policy there.
//   k_rs_inorder   inorder_contig<NL, IO_T, MASKED = true>: the reference's parent rule on G_F.
//   k_rs_fin       per contig: status, delta = float(D_F - D) / 1000.0, the record the host reads.
// The pinned re-annotation (§16: keep a chosen set of ORFs) is the same chain for the contigs that have required ORFs: k_rs_mask sets their
// edges' bits in a second bitmap and counts them, k_rc_lds / k_rc_inorder run the sweep and the parent rule under the REQ policy on one limb
// more, k_rs_fin splits the target's distance into the count of required edges and the W-sum.
// The evidence-weighted re-annotation (§19: a signed integer B per ORF added to its edge) is the chain a third time, for the contigs that
// have biased ORFs: k_ev_mask writes B to the edge's slot and sets its bit in a third bitmap, k_ev_lds / k_ev_inorder run the sweep and the
// parent rule under the BIAS policy in the contig's own class, k_ev_fin writes the record.
// The combined re-annotation (§22: required and biased ORFs in one solve) is the chain a fourth time, for the contigs that have both:
// k_rce_mask, k_rce_lds / k_rce_inorder under REQ and BIAS together on one limb more, k_rce_fin.
// The bitmap only ever holds bits of explicit rows: an ORF edge runs open -> close and a coded gap edge (a connector) close -> open, so no
// ORF shares both ends with a coded row, and k_rs_mask skips coded rows besides.  k_rs_lds therefore tests explicit rows only, and the
// masked inorder_contig, which tests every row, sees the same graph.
// Bounds: the sweep and round caps of k_sssp_lds (PHX_S_NEGCYCLE), no waiting between workgroups, no index from the caller on the device
// (the host checks the offsets; `forb` is one byte per ORF of the batch, `sel` one int per contig).

template <int NL> struct RsCfg { static constexpr int RING = 1024, ECAP = 1024; static constexpr bool MASKED = true, REQ = false, BIAS = false, BLIST = false; };
template <> struct RsCfg<17> { static constexpr int RING = 256, ECAP = 512; static constexpr bool MASKED = true, REQ = false, BIAS = false, BLIST = false; }; // 1088 bits: 109 KB of LDS instead of 283
template <int NL>
__host__ __device__ constexpr size_t rs_lds_bytes() { return (size_t)(RsCfg<NL>::RING + 1) * NL * 8 + (size_t)RsCfg<NL>::ECAP * ((size_t)NL * 8 + 4) + RS_PLAN_LDS + 64; }

__global__ __launch_bounds__(NT) void k_rs_mask(DBatch b, DReann q) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!(q.sel[blockIdx.x] | q.pin[blockIdx.x]) || !mg_contig(meta)) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const uint8_t *forb = q.forb + meta->orf_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const int V = meta->n_node;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const uint8_t f = forb[k];
        if (!f) continue;
        const DOrf o = orf[k];
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn; // start -> stop on the forward strand, stop -> start on the reverse (functions.py:310-316)
        if (u < 0 || v < 0 || u >= V || v >= V) continue;
        for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
            if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { // (no such edge: the ORF is ignored)
                atomicOr(&(f == 2 ? q.req : q.mask)[(ebase + x) >> 5], 1u << ((ebase + x) & 31));
                if (f == 2) atomicAdd(&q.kreq[blockIdx.x], 1); // k of §16: the required edges that exist
                break;
            }
    }
}

template <int NL>
// (five wavefronts per SIMD in the 128-bit class — two workgroups per CU where k_sssp_lds has three —: at k_sssp_lds' six the mask word and
// the row decoding cost ten spilled registers)
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 5 : (NL == 4 ? 4 : 2)) void k_rs_lds(DBatch b, DReann q) {
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (!q.sel[blockIdx.x] || !mg_contig(meta) || meta->sssp_nl != NL) return; // (no `overflow` test: the totals are the re-annotation's own, zeroed per call)
    lds_sweep<NL, RsCfg<NL>>(b, meta, blockIdx.x, V, q.mask, q.gplan);
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_rs_inorder(DBatch b, DReann q) {
    __shared__ IoShared<IO_T> sh;
    DMeta *meta = &b.meta[blockIdx.x];
    if (!q.sel[blockIdx.x] || meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return; // (a cycle of negative length: the solver has set the status)
    if (meta->n_path < 2 && meta->n_path != -1) return; // no path; -1: the walk along the lowest-index parents cycled
    inorder_contig<NL, IO_T, true>(b, meta, blockIdx.x, &sh, q.mask);
}

// ---- the pinned re-annotation (DESIGN.md §16): the contigs with required ORFs, DReann.pin ----
// A contig of limb class NL is solved in NL + 1 limbs with M = 2^(64 NL): a required edge weighs W - M, so the top limb of a distance is
// minus the count of required edges on its path (less one while the W-sum below is negative: rq_count) and the low NL limbs are the W-sum
// in the contig's own class, which obeys the layout's bound as before.  Counts are <= V < 2^30, far from the unreached pattern's 2^62.
// The ring of the 320-bit solve is halved (66 KB of LDS, two workgroups per CU, where 1024 entries would leave one).
template <int NL1> struct RcCfg { static constexpr int RING = 1024, ECAP = 1024; static constexpr bool MASKED = true, REQ = true, BIAS = false, BLIST = false; };
template <> struct RcCfg<5> { static constexpr int RING = 512, ECAP = 1024; static constexpr bool MASKED = true, REQ = true, BIAS = false, BLIST = false; };
template <> struct RcCfg<18> { static constexpr int RING = 256, ECAP = 512; static constexpr bool MASKED = true, REQ = true, BIAS = false, BLIST = false; };
template <int NL1>
__host__ __device__ constexpr size_t rc_lds_bytes() { return (size_t)(RcCfg<NL1>::RING + 1) * NL1 * 8 + (size_t)RcCfg<NL1>::ECAP * ((size_t)NL1 * 8 + 4) + RS_PLAN_LDS + 64; }

// NL: the contig's class; the sweep runs on NL + 1 limbs
template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 4 : 2) void k_rc_lds(DBatch b, DReann q) {
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (!q.pin[blockIdx.x] || !mg_contig(meta) || meta->sssp_nl != NL) return;
    lds_sweep<NL + 1, RcCfg<NL + 1>>(b, meta, blockIdx.x, V, q.mask, q.gplan, q.req, q.kreq[blockIdx.x]);
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_rc_inorder(DBatch b, DReann q) {
    __shared__ IoShared<IO_T> sh;
    DMeta *meta = &b.meta[blockIdx.x];
    if (!q.pin[blockIdx.x] || meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return;
    if (meta->n_path < 2 && meta->n_path != -1) return;
    inorder_contig<NL + 1, IO_T, true, true>(b, meta, blockIdx.x, &sh, q.mask, q.req);
}

// the count of required edges on the best path: the top limb of the NL + 1 limbs at df
template <int NL>
__device__ int64_t rc_count(const uint64_t *df) { return rq_count<NL + 1>(wi_load<NL + 1>(df)); }

template <int NL>
__device__ double rs_delta(const uint64_t *df, const uint64_t *d0) {
    const WInt<NL> DF = wi_load<NL>(df), D = wi_load<NL>(d0);
    return wi_to_double_rn<NL>(wi_add<NL>(DF, wi_neg<NL>(D))) / 1000.0; // float(D_F - D) / 1000.0 as §11-12 round it
}

// a thread per contig: the record the host reads
__global__ __launch_bounds__(64) void k_rs_fin(DBatch b, DReann q) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= b.n_contig || !(q.sel[c] | q.pin[c])) return;
    const DMeta *meta = &b.meta[c];
    DReannRec r;
    const bool pinned = q.pin[c] != 0;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    r.unmet = pinned ? q.nreq[c] : 0; r.pad_ = 0;
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        // the target's distance: the re-annotation's in its own stride (and one limb more when pinned: the W-sum is its low nl limbs), the run's in the run's
        const uint64_t *df = b.dist + (size_t)meta->node_off * b.dist_stride + (size_t)(V - 1) * (nl + (pinned ? 1 : 0));
        const uint64_t *d0 = q.dist0 + (size_t)meta->node_off * q.stride0 + (size_t)(V - 1) * nl;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        if (pinned) r.unmet -= (int32_t)(nl == 2 ? rc_count<2>(df) : nl == 4 ? rc_count<4>(df) : nl == 8 ? rc_count<8>(df) : rc_count<17>(df));
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    q.rec[c] = r;
}

// ---- the evidence-weighted re-annotation (DESIGN.md §19): the contigs with biased ORFs, DReann.evs ----
// The same chain once more under the BIAS policy, in the contig's own limb class: a biased ORF edge weighs W + B, B a signed 64-bit integer
// of the caller's (|B| <= 2^52, the host has checked it).  The values live in one word per in-edge slot of the batch (DReann.bval), never
// cleared: a word is read only where the slot's bit is set in DReann.bbit, which is cleared per call as `mask` and `req` are.  A bonus can
// make a cycle negative; the sweep's caps then end the solve as PHX_S_NEGCYCLE, exactly when the source reaches such a cycle (an unreached
// node is never relaxed).  The ring and tile sizes are k_rs_lds'.
template <int NL> struct EvCfg { static constexpr int RING = RsCfg<NL>::RING, ECAP = RsCfg<NL>::ECAP; static constexpr bool MASKED = true, REQ = false, BIAS = true, BLIST = false; };

// a thread per ORF of a contig that is solved under the bias policy: a refused or biased ORF finds its edge as in k_rs_mask; a refused one
// sets the slot's bit in `mask` (refusal wins over a bias), a biased one writes B to the slot's word, sets the slot's bit in `bbit` and
// adds |B| to the contig's sum — in two halves, which a contig's ORFs (< 2^31) cannot overflow
__global__ __launch_bounds__(NT) void k_ev_mask(DBatch b, DReann q) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!q.evs[blockIdx.x] || !mg_contig(meta)) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const uint8_t *forb = q.forb + meta->orf_off;
    const long long *bias = q.bias + meta->orf_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const int V = meta->n_node;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const uint8_t f = forb[k];
        const long long B = bias[k];
        if (f != 1 && B == 0) continue;
        const DOrf o = orf[k];
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn;
        if (u < 0 || v < 0 || u >= V || v >= V) continue;
        for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
            if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { // (no such edge: the ORF is ignored)
                if (f == 1) atomicOr(&q.mask[(ebase + x) >> 5], 1u << ((ebase + x) & 31));
                else {
                    const unsigned long long a = (unsigned long long)(B < 0 ? -B : B);
                    q.bval[ebase + x] = B;
                    atomicOr(&q.bbit[(ebase + x) >> 5], 1u << ((ebase + x) & 31));
                    atomicAdd(&q.bsum[2 * blockIdx.x], a & 0xffffffffull);
                    atomicAdd(&q.bsum[2 * blockIdx.x + 1], a >> 32);
                }
                break;
            }
    }
}

// (the launch bounds of k_rs_lds)
template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 5 : (NL == 4 ? 4 : 2)) void k_ev_lds(DBatch b, DReann q) {
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (!q.evs[blockIdx.x] || !mg_contig(meta) || meta->sssp_nl != NL) return;
    // the layout's bound plus the sum of |B|: beyond the contig's class there is no promotion, the contig ends before its sweep
    const double extra = (double)q.bsum[2 * blockIdx.x + 1] * 4294967296.0 + (double)q.bsum[2 * blockIdx.x];
    if (contig_sum_bits(b, meta, extra) > 64 * NL) {
        __syncthreads(); // (every thread has read the status)
        if (threadIdx.x == 0) { meta->status = PHX_S_OVERFLOW; meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0; }
        return;
    }
    lds_sweep<NL, EvCfg<NL>>(b, meta, blockIdx.x, V, q.mask, q.gplan, nullptr, 0, q.bbit, q.bval);
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_ev_inorder(DBatch b, DReann q) {
    __shared__ IoShared<IO_T> sh;
    DMeta *meta = &b.meta[blockIdx.x];
    if (!q.evs[blockIdx.x] || meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return; // (a cycle of negative length, or the biased bound beyond the class: the solver has set the status)
    if (meta->n_path < 2 && meta->n_path != -1) return;
    inorder_contig<NL, IO_T, true, false, true>(b, meta, blockIdx.x, &sh, q.mask, nullptr, q.bbit, q.bval);
}

// a thread per contig: the record the host reads (k_rs_fin's; delta = float(D_B - D) / 1000.0 may be negative, wi_to_double_rn rounds the
// magnitude to nearest-even and puts the sign back, which is what float() of a negative python integer does)
__global__ __launch_bounds__(64) void k_ev_fin(DBatch b, DReann q) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= b.n_contig || !q.evs[c]) return;
    const DMeta *meta = &b.meta[c];
    DReannRec r;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    r.unmet = 0; r.pad_ = 0;
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        const uint64_t *df = b.dist + (size_t)meta->node_off * b.dist_stride + (size_t)(V - 1) * nl;
        const uint64_t *d0 = q.dist0 + (size_t)meta->node_off * q.stride0 + (size_t)(V - 1) * nl;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    q.rec[c] = r;
}

// ---- the combined re-annotation (DESIGN.md §22): the contigs with required AND biased ORFs, DReann.rce ----
// Both policies in one solve: a row weighs W + B - M·[required], M = 2^(64 NL), on NL + 1 limbs as in §16.  The low NL limbs of a distance
// hold a sum of W + B, which k_rce_lds bounds by §19's limb test before the sweep, so M exceeds every walk sum and the top limb is the
// count of required edges as before (rq_count).  Both ends stay guarded: the count guard ends a solve whose source reaches a cycle through a
// required edge, the sweep and round caps one whose biases make a reachable cycle negative.  The ring and tile sizes are k_rc_lds'.
template <int NL1> struct RcEvCfg { static constexpr int RING = RcCfg<NL1>::RING, ECAP = RcCfg<NL1>::ECAP; static constexpr bool MASKED = true, REQ = true, BIAS = true, BLIST = false; };

// a thread per ORF of a contig that is solved under both policies: k_rs_mask's and k_ev_mask's marks in one pass.  A refused ORF sets its
// slot's bit in `mask` and nothing else; a required one sets the bit in `req` and counts for kreq; a biased one (required or not) writes B,
// sets the bit in `bbit` and adds |B| to the contig's sums.  Only explicit rows are marked; `forb` and `bias` are indexed by the contig's own
// ORFs, u and v are checked against V.
__global__ __launch_bounds__(NT) void k_rce_mask(DBatch b, DReann q) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!q.rce[blockIdx.x] || !mg_contig(meta)) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const uint8_t *forb = q.forb + meta->orf_off;
    const long long *bias = q.bias + meta->orf_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const int V = meta->n_node;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const uint8_t f = forb[k];
        const long long B = bias[k];
        if (!f && B == 0) continue;
        const DOrf o = orf[k];
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn;
        if (u < 0 || v < 0 || u >= V || v >= V) continue;
        for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
            if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { // (no such edge: the ORF is ignored, a required one stays unmet)
                const uint32_t bit = 1u << ((ebase + x) & 31);
                if (f == 1) { atomicOr(&q.mask[(ebase + x) >> 5], bit); break; } // refusal wins over a bias
                if (f == 2) { atomicOr(&q.req[(ebase + x) >> 5], bit); atomicAdd(&q.kreq[blockIdx.x], 1); }
                if (B != 0) {
                    const unsigned long long a = (unsigned long long)(B < 0 ? -B : B);
                    q.bval[ebase + x] = B;
                    atomicOr(&q.bbit[(ebase + x) >> 5], bit);
                    atomicAdd(&q.bsum[2 * blockIdx.x], a & 0xffffffffull);
                    atomicAdd(&q.bsum[2 * blockIdx.x + 1], a >> 32);
                }
                break;
            }
    }
}

// NL: the contig's class; the sweep runs on NL + 1 limbs behind k_ev_lds' limb test (the launch bounds of k_rc_lds)
template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 4 : 2) void k_rce_lds(DBatch b, DReann q) {
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (!q.rce[blockIdx.x] || !mg_contig(meta) || meta->sssp_nl != NL) return;
    // the sums of W + B must fit the contig's own class: M = 2^(64 NL) then exceeds every one of them
    const double extra = (double)q.bsum[2 * blockIdx.x + 1] * 4294967296.0 + (double)q.bsum[2 * blockIdx.x];
    if (contig_sum_bits(b, meta, extra) > 64 * NL) {
        __syncthreads(); // (every thread has read the status)
        if (threadIdx.x == 0) { meta->status = PHX_S_OVERFLOW; meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0; }
        return;
    }
    lds_sweep<NL + 1, RcEvCfg<NL + 1>>(b, meta, blockIdx.x, V, q.mask, q.gplan, q.req, q.kreq[blockIdx.x], q.bbit, q.bval);
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_rce_inorder(DBatch b, DReann q) {
    __shared__ IoShared<IO_T> sh;
    DMeta *meta = &b.meta[blockIdx.x];
    if (!q.rce[blockIdx.x] || meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return; // (a cycle, or the biased bound beyond the class: the solver has set the status)
    if (meta->n_path < 2 && meta->n_path != -1) return;
    inorder_contig<NL + 1, IO_T, true, true, true>(b, meta, blockIdx.x, &sh, q.mask, q.req, q.bbit, q.bval);
}

// a thread per contig: the record the host reads — delta from the low nl limbs of the target's distance (a sum of W + B, so it may be
// negative as in k_ev_fin), unmet from the top limb (k_rs_fin's pinned part)
__global__ __launch_bounds__(64) void k_rce_fin(DBatch b, DReann q) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= b.n_contig || !q.rce[c]) return;
    const DMeta *meta = &b.meta[c];
    DReannRec r;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    r.unmet = q.nreq[c]; r.pad_ = 0;
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        const uint64_t *df = b.dist + (size_t)meta->node_off * b.dist_stride + (size_t)(V - 1) * (nl + 1);
        const uint64_t *d0 = q.dist0 + (size_t)meta->node_off * q.stride0 + (size_t)(V - 1) * nl;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        r.unmet -= (int32_t)(nl == 2 ? rc_count<2>(df) : nl == 4 ? rc_count<4>(df) : nl == 8 ? rc_count<8>(df) : rc_count<17>(df));
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    q.rec[c] = r;
}

// ---- scenario batches (DESIGN.md §17): S masked re-annotations of the batch last run side by side, one workgroup per scenario slot ----
// A slot is one (contig, refused set).  Its kernels are the masked re-annotation's device functions — lds_sweep under RsCfg, inorder_contig
// with MASKED, emit_genes — entered with the slot's contig as their contig index (`ci`: the in_off row, the gap table and the global plan
// slice hang on it) and with the slot's view of the batch: the graph arrays are the run's, read only and shared by all slots of a contig;
// the per-contig record is the slot's own copy (DScen.meta), and the output pointers of the by-value DBatch are moved to where the
// contig's `node_off` lands on the slot's slices of dist / parent / path — what reann_batch does for the re-annotation as a whole, per
// slot.  Bitmap and plan pointers are shifted the same way (bit edge_off + e, byte node_off / 32 + ci).  Gene records come from the
// chunk's shared counter as in §14; the tie scratch from the chunk's bump allocator (DTotals.tie_need).

// a thread block per slot: the slot's copy of its contig's record, as the run left it
__global__ __launch_bounds__(64) void k_sc_meta(DBatch b, DScen q) {
    const int s = (int)blockIdx.x;
    const int c = q.slot[s].contig;
    if (c < 0 || c >= b.n_contig) return; // (the host has checked it)
    const uint64_t *from = (const uint64_t *)&b.meta[c];
    uint64_t *to = (uint64_t *)&q.meta[s];
    static_assert(sizeof(DMeta) % 8 == 0, "DMeta is copied in 64-bit words");
    for (int k = (int)threadIdx.x; k < (int)(sizeof(DMeta) / 8); k += 64) to[k] = from[k];
}

// a thread per listed (slot, ORF) pair: the ORF's edge, found as k_rs_mask finds it, sets its bit in the slot's bitmap slice
__global__ __launch_bounds__(NT) void k_sc_mask(DBatch b, DScen q) {
    const int64_t p = (int64_t)blockIdx.x * NT + (int64_t)threadIdx.x;
    if (p >= q.n_pair) return;
    const int2 pr = q.pair[p];
    if (pr.x < 0 || pr.x >= q.n_slot) return;
    const DScSlot sl = q.slot[pr.x];
    if (sl.contig < 0 || sl.contig >= b.n_contig) return;
    const DMeta *meta = &b.meta[sl.contig];
    const int k = pr.y;
    if (!mg_contig(meta) || k < 0 || k >= meta->n_orf) return;
    const DOrf o = b.orf[meta->orf_off + k];
    const int V = meta->n_node;
    const int sn = b.onode[meta->orf_off + k], tn = b.grp[meta->grp_off + o.grp].node;
    const bool fwd = o.frame > 0;
    const int u = fwd ? sn : tn, v = fwd ? tn : sn;
    if (u < 0 || v < 0 || u >= V || v >= V) return;
    const uint32_t *in_off = b.in_off + meta->node_off + sl.contig;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t lo = (uint64_t)meta->edge_off & 31u; // the slice keeps edge_off's position in a word
    for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
        if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { // (no such edge: the ORF is ignored)
            atomicOr(&q.mask[sl.mask0 + (int64_t)((lo + x) >> 5)], 1u << ((lo + x) & 31));
            break;
        }
}

// The slot's view of the batch (above).  Returns the slot's record; *ci its contig, *mask and *gplan what lds_sweep / inorder_contig index
// with edge_off + e and node_off / 32 + ci.
__device__ __forceinline__ DMeta *sc_view(DBatch &b, const DScen &q, uint32_t *ci, const uint32_t **mask, uint8_t **gplan) {
    const DScSlot sl = q.slot[blockIdx.x];
    DMeta *meta = &q.meta[blockIdx.x];
    const int64_t node_off = meta->node_off;
    b.dist = q.dist + (sl.dist0 - node_off * b.dist_stride);
    b.parent = q.parent + (sl.node0 - node_off);
    b.path = q.path + (sl.node0 - node_off);
    *ci = (uint32_t)sl.contig;
    *mask = q.mask + (sl.mask0 - (meta->edge_off >> 5));
    *gplan = q.gplan + (sl.plan0 - (node_off >> 5) - (int64_t)sl.contig);
    return meta;
}

template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 5 : (NL == 4 ? 4 : 2)) void k_sc_lds(DBatch b, DScen q) { // (the bounds of k_rs_lds)
    const uint32_t *mask;
    uint8_t *gplan;
    uint32_t ci;
    DMeta *meta = sc_view(b, q, &ci, &mask, &gplan);
    const int V = meta->n_node;
    if (!mg_contig(meta) || meta->sssp_nl != NL) return;
    lds_sweep<NL, RsCfg<NL>>(b, meta, ci, V, mask, gplan);
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_sc_inorder(DBatch b, DScen q) {
    __shared__ IoShared<IO_T> sh;
    const uint32_t *mask;
    uint8_t *gplan;
    uint32_t ci;
    DMeta *meta = sc_view(b, q, &ci, &mask, &gplan);
    if (meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return;
    if (meta->n_path < 2 && meta->n_path != -1) return;
    inorder_contig<NL, IO_T, true>(b, meta, ci, &sh, mask);
}

// a thread per slot: the record the host reads (k_rs_fin's, without the pinned part).  Also launched on the biased tail of the slot table
// (§20, phxk_scen_ev_finish): a biased slot's record is this one word for word, so a change here changes those slots too.
__global__ __launch_bounds__(64) void k_sc_fin(DBatch b, DScen q) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= q.n_slot) return;
    const DMeta *meta = &q.meta[s];
    DReannRec r;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    r.unmet = 0; r.pad_ = 0;
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        const uint64_t *df = q.dist + q.slot[s].dist0 + (size_t)(V - 1) * nl;
        const uint64_t *d0 = q.dist0 + (size_t)meta->node_off * q.stride0 + (size_t)(V - 1) * nl;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    q.rec[s] = r;
}

// ---- pinned scenario batches (DESIGN.md §18): the slots with required ORFs, solved under the REQ policy on one limb more ----
// The host puts the pinned slots behind the plain ones in a chunk's slot table and hands these kernels the table's tail (DScen.slot, meta,
// rec, req0, nreq, kreq moved to the first pinned slot, n_slot the pinned slots), so that blockIdx.x is a pinned slot here as it is a plain
// one in k_sc_*, whose grids end where these begin.  The distance slice of a pinned slot holds n_node x (NL + 1) words; its refused slice
// is set by k_sc_mask like any slot's, its required slice (DScen.req at req0, the same bit rule) by k_scp_mask.

// a thread per required (slot, ORF) pair of the chunk (slot: its index in the whole table): the ORF's edge, found as k_sc_mask finds it,
// sets its bit in the slot's required slice and counts for the slot's kreq, the k of the solver's cycle guard
__global__ __launch_bounds__(NT) void k_scp_mask(DBatch b, DScen q) {
    const int64_t p = (int64_t)blockIdx.x * NT + (int64_t)threadIdx.x;
    if (p >= q.n_rpair) return;
    const int2 pr = q.rpair[p];
    if (pr.x < 0 || pr.x >= q.n_slot) return;
    const DScSlot sl = q.slot[pr.x];
    if (!sl.pinned || sl.contig < 0 || sl.contig >= b.n_contig) return;
    const DMeta *meta = &b.meta[sl.contig];
    const int k = pr.y;
    if (!mg_contig(meta) || k < 0 || k >= meta->n_orf) return;
    const DOrf o = b.orf[meta->orf_off + k];
    const int V = meta->n_node;
    const int sn = b.onode[meta->orf_off + k], tn = b.grp[meta->grp_off + o.grp].node;
    const bool fwd = o.frame > 0;
    const int u = fwd ? sn : tn, v = fwd ? tn : sn;
    if (u < 0 || v < 0 || u >= V || v >= V) return;
    const uint32_t *in_off = b.in_off + meta->node_off + sl.contig;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t lo = (uint64_t)meta->edge_off & 31u;
    for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
        if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { // (no such edge: the ORF stays unmet)
            const uint32_t bit = 1u << ((lo + x) & 31);
            if (!(atomicOr(&q.req[q.req0[pr.x] + (int64_t)((lo + x) >> 5)], bit) & bit)) atomicAdd(&q.kreq[pr.x], 1); // (an ORF listed twice counts once)
            break;
        }
}

// the slot's required slice, shifted by sc_view's rule
__device__ __forceinline__ const uint32_t *scp_req(const DScen &q, const DMeta *meta) { return q.req + (q.req0[blockIdx.x] - (meta->edge_off >> 5)); }

template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 4 : 2) void k_scp_lds(DBatch b, DScen q) { // (the bounds of k_rc_lds)
    const uint32_t *mask;
    uint8_t *gplan;
    uint32_t ci;
    DMeta *meta = sc_view(b, q, &ci, &mask, &gplan);
    const int V = meta->n_node;
    if (!mg_contig(meta) || meta->sssp_nl != NL) return;
    lds_sweep<NL + 1, RcCfg<NL + 1>>(b, meta, ci, V, mask, gplan, scp_req(q, meta), q.kreq[blockIdx.x]);
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_scp_inorder(DBatch b, DScen q) {
    __shared__ IoShared<IO_T> sh;
    const uint32_t *mask;
    uint8_t *gplan;
    uint32_t ci;
    DMeta *meta = sc_view(b, q, &ci, &mask, &gplan);
    if (meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return;
    if (meta->n_path < 2 && meta->n_path != -1) return;
    inorder_contig<NL + 1, IO_T, true, true>(b, meta, ci, &sh, mask, scp_req(q, meta));
}

// a thread per pinned slot: the record the host reads (k_rs_fin's pinned part, per slot)
__global__ __launch_bounds__(64) void k_scp_fin(DBatch b, DScen q) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= q.n_slot) return;
    const DMeta *meta = &q.meta[s];
    DReannRec r;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    r.unmet = q.nreq[s]; r.pad_ = 0;
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        const uint64_t *df = q.dist + q.slot[s].dist0 + (size_t)(V - 1) * (nl + 1); // the W-sum is the low nl limbs
        const uint64_t *d0 = q.dist0 + (size_t)meta->node_off * q.stride0 + (size_t)(V - 1) * nl;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        r.unmet -= (int32_t)(nl == 2 ? rc_count<2>(df) : nl == 4 ? rc_count<4>(df) : nl == 8 ? rc_count<8>(df) : rc_count<17>(df));
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    q.rec[s] = r;
}

// ---- evidence scenarios (DESIGN.md §20): the slots with biased ORFs, solved under the BIAS policy with a sparse list per slot ----
// The host puts the biased slots behind the plain and the pinned ones in a chunk's slot table and hands the solve and the finish the table's
// tail (DScen.slot, meta, rec, bs moved to the first biased slot, n_slot the biased slots), as §18 does for the pinned ones.  A biased slot
// keeps no word per in-edge slot (a dense slice would be 8 E bytes, more than everything else the slot owns): it has a bias bitmap slice
// (DScen.bbit at DScBias.bbit0, the bit rule of mask0) and a list of (in-edge slot of the batch, B) pairs sorted by in-edge slot, which the shared code
// searches where the slot's bit is set (bias_at under BLIST, phx_sssp.inc).  Its refused slice is set by k_sc_mask like any slot's.
template <int NL> struct EsCfg { static constexpr int RING = EvCfg<NL>::RING, ECAP = EvCfg<NL>::ECAP; static constexpr bool MASKED = true, REQ = false, BIAS = true, BLIST = true; };

// a thread per (slot, ORF, B) triple of the chunk (slot: its index in the whole table): the ORF's edge, found as k_sc_mask finds it, sets
// its bit in the slot's bias slice, appends (in-edge slot, B) to the slot's list and adds |B| to the slot's sums as k_ev_mask does.  A
// slot with one triple needs no sorting and appends to its list proper, any other to its staging area.
__global__ __launch_bounds__(NT) void k_sce_mask(DBatch b, DScen q) {
    const int64_t p = (int64_t)blockIdx.x * NT + (int64_t)threadIdx.x;
    if (p >= q.n_trip) return;
    const DScTrip tr = q.trip[p];
    if (tr.slot < 0 || tr.slot >= q.n_slot) return;
    const DScSlot sl = q.slot[tr.slot];
    if (sl.contig < 0 || sl.contig >= b.n_contig) return;
    const DMeta *meta = &b.meta[sl.contig];
    const int k = tr.orf;
    if (!mg_contig(meta) || k < 0 || k >= meta->n_orf) return;
    const DOrf o = b.orf[meta->orf_off + k];
    const int V = meta->n_node;
    const int sn = b.onode[meta->orf_off + k], tn = b.grp[meta->grp_off + o.grp].node;
    const bool fwd = o.frame > 0;
    const int u = fwd ? sn : tn, v = fwd ? tn : sn;
    if (u < 0 || v < 0 || u >= V || v >= V) return;
    const uint32_t *in_off = b.in_off + meta->node_off + sl.contig;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t lo = (uint64_t)meta->edge_off & 31u;
    DScBias *bs = &q.bs[tr.slot];
    for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
        if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { // (no such edge: the ORF is ignored)
            const int at = atomicAdd(&bs->cnt, 1);
            if (at >= bs->n_trip) break; // (the host sized the list by the slot's triples)
            atomicOr(&q.bbit[bs->bbit0 + (int64_t)((lo + x) >> 5)], 1u << ((lo + x) & 31));
            long long *to = (bs->n_trip == 1 ? q.blist : q.bstage) + 2 * (bs->list0 + at);
            to[0] = (long long)((uint64_t)meta->edge_off + x); to[1] = tr.B; // (the batch's in-edge slot, as the shared code counts them)
            const unsigned long long a = (unsigned long long)(tr.B < 0 ? -tr.B : tr.B);
            atomicAdd(&bs->bsum[0], a & 0xffffffffull);
            atomicAdd(&bs->bsum[1], a >> 32);
            break;
        }
}

// pairs a biased slot's list holds: what k_sce_mask appended, never beyond the list
__device__ __forceinline__ int sce_count(const DScBias &bs) { return bs.cnt < bs.n_trip ? bs.cnt : bs.n_trip; }

// the staged pairs of a biased slot into its list in ascending order of their in-edge slot.  A pair's place is the number of pairs in
// front of it (an equal in-edge slot: the one staged earlier), found by counting — a list is at most a contig's ORFs.  gridDim.y
// workgroups share a slot's pairs, NT at a time; the keys they count over pass through LDS in tiles of NT.
__global__ __launch_bounds__(NT) void k_sce_sort(DScen q) {
    __shared__ long long s_key[NT];
    const DScBias bs = q.bs[blockIdx.x];
    if (bs.n_trip <= 1) return; // (k_sce_mask wrote the list itself)
    const int n = sce_count(bs);
    const int tid = (int)threadIdx.x;
    const long long *from = q.bstage + 2 * bs.list0;
    long long *to = q.blist + 2 * bs.list0;
    for (int i0 = (int)blockIdx.y * NT; i0 < n; i0 += (int)gridDim.y * NT) { // (i0, n: the same in every thread, so are the barriers)
        const int i = i0 + tid;
        const long long key = i < n ? from[2 * i] : 0ll;
        int at = 0;
        for (int j0 = 0; j0 < n; j0 += NT) {
            __syncthreads();
            if (j0 + tid < n) s_key[tid] = from[2 * (j0 + tid)];
            __syncthreads();
            const int m = n - j0 < NT ? n - j0 : NT;
            for (int j = 0; j < m; j++) { const long long kj = s_key[j]; at += kj < key || (kj == key && j0 + j < i); }
        }
        if (i < n) { to[2 * at] = key; to[2 * at + 1] = from[2 * i + 1]; }
    }
}

// the slot's bias slice, shifted by sc_view's rule, and its list
__device__ __forceinline__ const uint32_t *sce_bbit(const DScen &q, const DScBias &bs, const DMeta *meta) { return q.bbit + (bs.bbit0 - (meta->edge_off >> 5)); }

template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 5 : (NL == 4 ? 4 : 2)) void k_sce_lds(DBatch b, DScen q) { // (the bounds of k_ev_lds)
    const uint32_t *mask;
    uint8_t *gplan;
    uint32_t ci;
    DMeta *meta = sc_view(b, q, &ci, &mask, &gplan);
    const int V = meta->n_node;
    if (!mg_contig(meta) || meta->sssp_nl != NL) return;
    const DScBias bs = q.bs[blockIdx.x];
    // k_ev_lds' limb-class test on the slot's sums
    const double extra = (double)bs.bsum[1] * 4294967296.0 + (double)bs.bsum[0];
    if (contig_sum_bits(b, meta, extra) > 64 * NL) {
        __syncthreads(); // (every thread has read the status)
        if (threadIdx.x == 0) { meta->status = PHX_S_OVERFLOW; meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0; }
        return;
    }
    lds_sweep<NL, EsCfg<NL>>(b, meta, ci, V, mask, gplan, nullptr, 0, sce_bbit(q, bs, meta), q.blist + 2 * bs.list0, sce_count(bs));
}

template <int NL, int IO_T>
__global__ __launch_bounds__(IO_T) void k_sce_inorder(DBatch b, DScen q) {
    __shared__ IoShared<IO_T> sh;
    const uint32_t *mask;
    uint8_t *gplan;
    uint32_t ci;
    DMeta *meta = sc_view(b, q, &ci, &mask, &gplan);
    if (meta->sssp_nl != NL) return;
    if (threadIdx.x == 0) { sh.flag = 0; meta->tie = 0; }
    __syncthreads();
    if (!mg_contig(meta)) return; // (a cycle of negative length, or the biased bound beyond the class: the solver has set the status)
    if (meta->n_path < 2 && meta->n_path != -1) return;
    const DScBias bs = q.bs[blockIdx.x];
    inorder_contig<NL, IO_T, true, false, true, true>(b, meta, ci, &sh, mask, nullptr, sce_bbit(q, bs, meta), q.blist + 2 * bs.list0, sce_count(bs));
}
// (the record of a biased slot is k_ev_fin's through the slot view, which is k_sc_fin's word for word: the finish launches k_sc_fin on the tail)
