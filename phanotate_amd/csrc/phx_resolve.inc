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
//   k_rs_lds<NL>   the windowed workgroup-per-contig sweep of k_sssp_lds over G_F: a refused edge enters the window's tile as "no edge"
//                  (weight = unreached, source = the constant-zero slot), so the phases pay nothing for the mask; the rows come through
//                  edge_wenc (coded gap edges from the contig's gap table: no k_edges_expand, nothing written to DBatch.ew).  The
//                  verification pass skips refused edges: they neither violate the fixed point nor become a parent.
//   k_rs_inorder   inorder_contig<NL, IO_T, MASKED = true>: the reference's parent rule on G_F.
//   k_rs_fin       per contig: status, delta = float(D_F - D) / 1000.0, the record the host reads.
// The bitmap only ever holds bits of explicit rows: an ORF edge runs open -> close and a coded gap edge (a connector) close -> open, so no
// ORF shares both ends with a coded row, and k_rs_mask skips coded rows besides.  k_rs_lds therefore tests explicit rows only, and the
// masked inorder_contig, which tests every row, sees the same graph.
// Bounds: the sweep and round caps of k_sssp_lds (PHX_S_NEGCYCLE), no waiting between workgroups, no index from the caller on the device
// (the host checks the offsets; `forb` is one byte per ORF of the batch, `sel` one int per contig).

#define RS_PLAN_LDS 2048 // window-plan bytes kept in LDS (contigs of up to 65 536 nodes); longer plans live in DReann.gplan

template <int NL> struct RsCfg { static constexpr int RING = 1024, ECAP = 1024; };
template <> struct RsCfg<17> { static constexpr int RING = 256, ECAP = 512; }; // 1088 bits: 109 KB of LDS instead of 283
template <int NL>
__host__ __device__ constexpr size_t rs_lds_bytes() { return (size_t)(RsCfg<NL>::RING + 1) * NL * 8 + (size_t)RsCfg<NL>::ECAP * ((size_t)NL * 8 + 4) + RS_PLAN_LDS + 64; }

__device__ __forceinline__ bool rs_refused(const uint32_t *mask, uint64_t ebase, uint32_t e) {
    const uint64_t x = ebase + e;
    return ((mask[x >> 5] >> (x & 31)) & 1u) != 0;
}

__global__ __launch_bounds__(NT) void k_rs_mask(DBatch b, DReann q) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!q.sel[blockIdx.x] || !mg_contig(meta)) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const uint8_t *forb = q.forb + meta->orf_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const int V = meta->n_node;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        if (!forb[k]) continue;
        const DOrf o = orf[k];
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn; // start -> stop on the forward strand, stop -> start on the reverse (functions.py:310-316)
        if (u < 0 || v < 0 || u >= V || v >= V) continue;
        for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
            if (!ESRC_IS_GAP(esrc[x]) && ESRC_NODE(esrc[x]) == (uint32_t)u) { atomicOr(&q.mask[(ebase + x) >> 5], 1u << ((ebase + x) & 31)); break; } // (no such edge: the ORF is ignored)
    }
}

// k_sssp_lds (phx_sssp.inc) over G_F; see there for the window scheme.  The body is that kernel's, statement for statement; a fix to the
// window scheme there belongs here too.  The places that differ, and nothing else does:
//   * entry: the contig is chosen by DReann.sel and mg_contig, not by sssp_mode / lds_given / sweeps; no `overflow` test (the totals are the
//     re-annotation's own, zeroed per call); no expand_contig, SW_CENSUS or SW_PROFILE;
//   * sizes: SW_RING / SW_ECAP / SW_EPT are RsCfg<NL>::RING / ECAP and EPT; `plan` is in LDS up to RS_PLAN_LDS windows, else in DReann.gplan,
//     and plan[k + 1], plan[k + 2] are read once at the head of a window (nwn1, nwn2);
//   * rows: the prologue and the prefetch of window k + 1 keep the source NODE in r_src and read the weight through edge_wenc; bit j of r_mk
//     says that tile edge j of this thread is an explicit row whose mask bit is set;
//   * tile commit: such an edge gets weight = `big` (the unreached pattern) and the constant-zero slot;
//   * the untiled loop and the verification pass read the row through edge_wenc and `continue` on a refused explicit row;
//   * the end: gene slots always come from the shared counter (no gpack).
template <int NL>
// (five wavefronts per SIMD in the 128-bit class — two workgroups per CU where k_sssp_lds has three —: at k_sssp_lds' six the mask word and
// the row decoding cost ten spilled registers)
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? 5 : (NL == 4 ? 4 : 2)) void k_rs_lds(DBatch b, DReann q) {
    constexpr int RING = RsCfg<NL>::RING, ECAP = RsCfg<NL>::ECAP;
    constexpr int EPT = (ECAP + SW_THREADS - 1) / SW_THREADS;
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int s_flag[2];
    __shared__ int s_np, s_nclose, s_viol;
    __shared__ uint32_t s_off[2][SW_MAX + 1];
    __shared__ uint8_t s_list[SW_MAX];
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (!q.sel[blockIdx.x] || !mg_contig(meta) || meta->sssp_nl != NL) return;
    const int tid = threadIdx.x;
    const int SRC = V - 2, TGT = V - 1, ncds = V - 2;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const uint32_t *mask = q.mask;
    const DNode *nd = b.node + meta->node_off;
    uint64_t *gdist = b.dist + (size_t)meta->node_off * b.dist_stride;
    uint64_t *ring = (uint64_t *)smem;
    uint64_t *tw = ring + (size_t)(RING + 1) * NL;
    uint32_t *tsrc = (uint32_t *)(tw + (size_t)ECAP * NL);
    const size_t lds_words = (size_t)(RING + 1) * NL * 2 + (size_t)ECAP * NL * 2 + ECAP; // 32-bit words before the plan
    const int nW = (V + SW_ADV - 1) / SW_ADV;
    uint8_t *plan = nW <= RS_PLAN_LDS ? (uint8_t *)(tsrc + ECAP) : q.gplan + (size_t)(meta->node_off >> 5) + blockIdx.x; // (a contig's slice: >= V / 32 + 1 bytes)
    for (int v = tid; v < V; v += SW_THREADS) {
        WInt<NL> d;
#pragma unroll
        for (int i = 0; i < NL; i++) d.v[i] = 0;
        if (v != SRC) d.v[NL - 1] = WBIG_TOP;
        wi_store<NL>(gdist + (size_t)v * NL, d);
    }
    if (tid < NL) ring[(size_t)RING * NL + tid] = 0;
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
    for (int k = tid >> 6; k < nW; k += SW_THREADS / 64) {
        const int v0 = k * SW_ADV, lane = tid & 63;
        const int vadv = v0 + SW_ADV < V ? v0 + SW_ADV : V;
        const int idx = v0 + lane;
        bool ok = idx < V;
        if (ok && idx >= vadv) ok = idx < ncds && vadv - 1 < ncds && nd[idx].pos < nd[vadv - 1].pos + 500 && in_off[idx + 1] - in_off[v0] <= (uint32_t)ECAP;
        const uint64_t m = __ballot(ok);
        const int cnt = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
        if (lane == 0) plan[k] = (uint8_t)cnt;
    }
    __syncthreads();
    const int node_l = tid / SW_LPN, sub = tid % SW_LPN;
    int sweeps = 0, it = 0;
    bool again = true, bad = false;
    uint32_t *gpe = (uint32_t *)(b.parent + meta->node_off);
    const bool ps_lds = (size_t)V <= lds_words;
    uint32_t *psrc = (uint32_t *)smem;
    WInt<NL> big;
#pragma unroll
    for (int i = 0; i < NL; i++) big.v[i] = 0;
    big.v[NL - 1] = WBIG_TOP;
    while (again && !bad) {
        int loaded = 0;
        if (tid < NL) ring[(size_t)RING * NL + tid] = 0;
        if (tid == 0) s_viol = 0;
        __syncthreads();
        // registers that carry window k+1's data while window k iterates; bit j of r_mk: tile edge j of this thread is refused
        uint32_t r_src[EPT];
        long long r_w[EPT];
        uint32_t r_mk = 0;
        uint32_t r_offn = 0;
        int r_type = 0;
        WInt<NL> r_ring;
        {
            const int nw0 = plan[0];
            if (tid <= nw0) s_off[0][tid] = in_off[tid];
            __syncthreads();
            const uint32_t e0n = s_off[0][0];
            const int nen = (int)(s_off[0][nw0] - e0n);
            r_type = tid < nw0 ? nd[tid].info : 0;
            r_ring = wi_load<NL>(gdist + (size_t)(tid < nw0 ? tid : 0) * NL);
            r_offn = (nW > 1 && tid <= plan[1]) ? in_off[SW_ADV + tid] : 0u;
#pragma unroll
            for (int j = 0; j < EPT; j++) {
                const int i = tid + j * SW_THREADS;
                const bool on = nen <= ECAP && i < nen;
                const uint32_t sw = on ? esrc[e0n + i] : 0u;
                r_src[j] = ESRC_NODE(sw);
                r_w[j] = on ? edge_wenc(sw, ew, e0n + i, gt) : 0ll;
                if (on && !ESRC_IS_GAP(sw) && rs_refused(mask, ebase, e0n + i)) r_mk |= 1u << j;
            }
        }
        for (int k = 0; k < nW && !bad; k++) {
            const int cur = k & 1;
            const int v0 = k * SW_ADV;
            const int nwin = plan[k];
            const int v1 = v0 + nwin;
            const int nwn1 = k + 1 < nW ? plan[k + 1] : 0, nwn2 = k + 2 < nW ? plan[k + 2] : 0;
            if (k + 1 < nW && tid <= nwn1) s_off[cur ^ 1][tid] = r_offn;
            if (tid < 64) {
                const int t = NTYPE(r_type), f = NFRAME(r_type);
                const bool isclose = tid < nwin && ((t == 1 && f > 0) || (t == 0 && f < 0));
                const uint64_t mc = __ballot(isclose);
                const uint64_t mo = __ballot(tid < nwin && !isclose);
                const uint64_t below = tid ? (~0ull >> (64 - tid)) : 0ull;
                const int nc = __popcll(mc);
                if (tid < nwin) s_list[isclose ? __popcll(mc & below) : nc + __popcll(mo & below)] = (uint8_t)tid;
                if (tid == 0) s_nclose = nc;
            }
            if (loaded + tid < v1) wi_store<NL>(ring + (size_t)((loaded + tid) & (RING - 1)) * NL, r_ring);
            loaded = v1 > loaded ? v1 : loaded;
            const uint32_t e0 = s_off[cur][0];
            const int ne = (int)(s_off[cur][nwin] - e0);
            const bool tiled = ne <= ECAP;
            if (tiled) {
#pragma unroll
                for (int j = 0; j < EPT; j++) {
                    const int i = tid + j * SW_THREADS;
                    if (i < ne) {
                        const uint32_t u = r_src[j];
                        WInt<NL> w = ew_decode<NL>(r_w[j]);
                        uint32_t sl = RING;
                        if ((r_mk >> j) & 1u) w = big; // refused: no edge (0 + "unreached" never wins)
                        else if (u != (uint32_t)SRC) {
                            if ((int)u < loaded && (int)u + RING >= loaded) sl = u & (RING - 1);
                            else w = wi_add<NL>(w, wi_load<NL>(gdist + (size_t)u * NL));
                        }
                        tsrc[i] = sl;
                        wi_store<NL>(tw + (size_t)i * NL, w);
                    }
                }
            }
            __syncthreads();
            if (k + 1 < nW) {
                const int v0n = v0 + SW_ADV, nwn = nwn1, v1n = v0n + nwn;
                const uint32_t e0n = s_off[cur ^ 1][0];
                const int nen = (int)(s_off[cur ^ 1][nwn] - e0n);
                r_type = tid < nwn ? nd[v0n + tid].info : 0;
                r_ring = wi_load<NL>(gdist + (size_t)(loaded + tid < v1n ? loaded + tid : 0) * NL);
                r_offn = (k + 2 < nW && tid <= nwn2) ? in_off[v0n + SW_ADV + tid] : 0u;
                r_mk = 0;
#pragma unroll
                for (int j = 0; j < EPT; j++) {
                    const int i = tid + j * SW_THREADS;
                    const bool on = nen <= ECAP && i < nen;
                    const uint32_t sw = on ? esrc[e0n + i] : 0u;
                    r_src[j] = ESRC_NODE(sw);
                    r_w[j] = on ? edge_wenc(sw, ew, e0n + i, gt) : 0ll;
                    if (on && !ESRC_IS_GAP(sw) && rs_refused(mask, ebase, e0n + i)) r_mk |= 1u << j;
                }
            }
            const int nclose = s_nclose, nopen = nwin - nclose;
            const bool actA = node_l < nclose, actB = node_l < nopen;
            const int lA = actA ? s_list[node_l] : 0, lB = actB ? s_list[nclose + node_l] : 0;
            const int iaA = actA ? (int)(s_off[cur][lA] - e0) + sub : 0, ibA = actA ? (int)(s_off[cur][lA + 1] - e0) : 0;
            const int iaB = actB ? (int)(s_off[cur][lB] - e0) + sub : 0, ibB = actB ? (int)(s_off[cur][lB + 1] - e0) : 0;
            uint64_t *slotA = ring + (size_t)((v0 + lA) & (RING - 1)) * NL, *slotB = ring + (size_t)((v0 + lB) & (RING - 1)) * NL;
            uint64_t *gA = gdist + (size_t)(v0 + lA) * NL, *gB = gdist + (size_t)(v0 + lB) * NL;
            uint32_t csA[SW_RCA], csB[SW_RCB];
            WInt<NL> cwA[SW_RCA], cwB[SW_RCB];
#pragma unroll
            for (int j = 0; j < SW_RCA; j++) {
                const int ia = iaA + j * SW_LPN;
                const bool oa = tiled && ia < ibA;
                csA[j] = oa ? tsrc[ia] : (uint32_t)RING;
                cwA[j] = oa ? wi_load<NL>(tw + (size_t)ia * NL) : big;
            }
#pragma unroll
            for (int j = 0; j < SW_RCB; j++) {
                const int ib = iaB + j * SW_LPN;
                const bool ob = tiled && ib < ibB;
                csB[j] = ob ? tsrc[ib] : (uint32_t)RING;
                cwB[j] = ob ? wi_load<NL>(tw + (size_t)ib * NL) : big;
            }
            int inner = 0;
            for (int ph = 0;; ph ^= 1) {
                const bool act = ph ? actB : actA;
                if ((tid & ~63) / SW_LPN < (ph ? nopen : nclose)) {
                    const int ia = ph ? iaB : iaA, ib = ph ? ibB : ibA;
                    uint64_t *myslot = ph ? slotB : slotA;
                    WInt<NL> d0 = big;
                    if (act) d0 = wi_load<NL>(myslot);
                    WInt<NL> best = d0;
                    if (tiled) {
                        int i;
                        if (ph) {
#pragma unroll
                            for (int j = 0; j < SW_RCB; j++) best = wi_min_bf<NL>(best, wi_add<NL>(wi_load<NL>(ring + (size_t)csB[j] * NL), cwB[j]));
                            i = ia + SW_RCB * SW_LPN;
                        } else {
#pragma unroll
                            for (int j = 0; j < SW_RCA; j++) best = wi_min_bf<NL>(best, wi_add<NL>(wi_load<NL>(ring + (size_t)csA[j] * NL), cwA[j]));
                            i = ia + SW_RCA * SW_LPN;
                        }
                        uint32_t sl = i < ib ? tsrc[i] : 0u;
                        while (i < ib) {
                            const int in = i + SW_LPN;
                            const uint32_t sn = in < ib ? tsrc[in] : 0u;
                            best = wi_min_bf<NL>(best, wi_add<NL>(wi_load<NL>(ring + (size_t)sl * NL), wi_load<NL>(tw + (size_t)i * NL)));
                            sl = sn;
                            i = in;
                        }
                    } else {
                        for (int i = ia; i < ib; i += SW_LPN) {
                            const uint32_t sw = esrc[e0 + i];
                            if (!ESRC_IS_GAP(sw) && rs_refused(mask, ebase, e0 + i)) continue;
                            const uint32_t u = ESRC_NODE(sw);
                            WInt<NL> du;
                            if (u == (uint32_t)SRC) du = wi_load<NL>(ring + (size_t)RING * NL);
                            else if ((int)u < loaded && (int)u + RING >= loaded) du = wi_load<NL>(ring + (size_t)(u & (RING - 1)) * NL);
                            else du = wi_load<NL>(gdist + (size_t)u * NL);
                            best = wi_min_bf<NL>(best, wi_add<NL>(du, ew_decode<NL>(edge_wenc(sw, ew, e0 + i, gt))));
                        }
                    }
                    best = wi_row_min<NL>(best, sub);
                    if (act && sub == SW_LPN - 1 && wi_lt_bf<NL>(best, d0)) {
                        wi_store<NL>(myslot, best);
                        wi_store<NL>(ph ? gB : gA, best); // write-through
                        s_flag[it & 1] = 1;
                    }
                }
                if (tid == 0) s_flag[(it + 1) & 1] = 0;
                __syncthreads();
                const bool chg = s_flag[it & 1] != 0;
                it++;
                if (!chg && (ph == 1 || inner > 0)) break;
                if (++inner > 2 * SW_MAX + 16) { bad = true; break; }
            }
        }
        if (++sweeps > V + 2) bad = true;
        __syncthreads();
        // verification + parents over the edges of G_F: a refused edge neither violates the fixed point nor becomes a parent
        for (int vb = 0; vb < V; vb += SW_MAX) {
            const int v = vb + node_l;
            uint32_t be = PE_NONE;
            bool viol = false;
            if (v < V) {
                const WInt<NL> dv = wi_load<NL>(gdist + (size_t)v * NL);
                const uint32_t e1 = in_off[v + 1];
                for (uint32_t e = in_off[v] + sub; e < e1; e += SW_LPN) {
                    const uint32_t sw = esrc[e];
                    if (!ESRC_IS_GAP(sw) && rs_refused(mask, ebase, e)) continue;
                    const WInt<NL> cand = wi_add<NL>(wi_load<NL>(gdist + (size_t)ESRC_NODE(sw) * NL), ew_decode<NL>(edge_wenc(sw, ew, e, gt)));
                    if (wi_lt_bf<NL>(cand, dv)) viol = true;
                    if (wi_eq<NL>(cand, dv) && e < be && !wi_unreached<NL>(dv)) be = e;
                }
            }
            be = u32_row_min(be, sub);
            if (viol) s_viol = 1;
            if (v < V && sub == SW_LPN - 1) { gpe[v] = be; if (ps_lds) psrc[v] = be == PE_NONE ? PE_NONE : ESRC_NODE(esrc[be]); }
        }
        __syncthreads();
        again = s_viol != 0;
        __syncthreads();
    }
    // path and genes, as k_sssp_lds (phanotate.py:64-76), into the re-annotation's own buffers
    int32_t *path = b.path + meta->node_off;
    if (tid == 0) {
        meta->sweeps = sweeps;
        meta->sssp_iters = it;
        meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0;
        int np = -1;
        if (bad) meta->status = PHX_S_NEGCYCLE;
        else if (wi_unreached<NL>(wi_load<NL>(gdist + (size_t)TGT * NL))) meta->status = PHX_S_NOPATH;
        else {
            int n = 0;
            for (int v = TGT; v != SRC && n <= V; v = ps_lds ? (int)psrc[v] : (int)ESRC_NODE(esrc[gpe[v]])) n++;
            if (n > V) meta->n_path = -1; // see emit_path_and_genes
            else {
                int k = n;
                for (int v = TGT;; v = ps_lds ? (int)psrc[v] : (int)ESRC_NODE(esrc[gpe[v]])) { path[k--] = v; if (v == SRC || k < 0) break; }
                meta->n_path = n + 1;
                np = n / 2;
                meta->n_genes = np;
                meta->gene_off = atomicAdd(b.gene_total, (uint32_t)np);
            }
        }
        s_np = np;
    }
    __syncthreads();
    const int npairs = s_np;
    if (npairs > 0) emit_genes(b, meta, path, npairs, (size_t)meta->gene_off, tid, SW_THREADS);
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
    inorder_contig<NL, IO_T, true>(b, meta, &sh, q.mask);
}

template <int NL>
__device__ double rs_delta(const uint64_t *df, const uint64_t *d0) {
    const WInt<NL> DF = wi_load<NL>(df), D = wi_load<NL>(d0);
    return wi_to_double_rn<NL>(wi_add<NL>(DF, wi_neg<NL>(D))) / 1000.0; // float(D_F - D) / 1000.0 as §11-12 round it
}

// a thread per contig: the record the host reads
__global__ __launch_bounds__(64) void k_rs_fin(DBatch b, DReann q) {
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= b.n_contig || !q.sel[c]) return;
    const DMeta *meta = &b.meta[c];
    DReannRec r;
    r.status = meta->status; r.n_genes = 0; r.gene_off = 0; r.n_path = 0; r.tie = meta->tie; r.delta = __builtin_inf();
    if (meta->status >= 0 && meta->status != PHX_S_NOPATH && meta->n_path >= 2) {
        const int V = meta->n_node, nl = meta->sssp_nl;
        const size_t t = (size_t)meta->node_off * b.dist_stride + (size_t)(V - 1) * nl;
        const uint64_t *df = b.dist + t, *d0 = q.dist0 + t;
        r.delta = nl == 2 ? rs_delta<2>(df, d0) : nl == 4 ? rs_delta<4>(df, d0) : nl == 8 ? rs_delta<8>(df, d0) : rs_delta<17>(df, d0);
        r.n_genes = meta->n_genes; r.gene_off = meta->gene_off; r.n_path = meta->n_path;
    }
    q.rec[c] = r;
}

template <int NL>
static void launch_rs_lds(const DBatch *b, const DReann *q, hipStream_t s) {
    const size_t lb = rs_lds_bytes<NL>();
    (void)hipFuncSetAttribute((const void *)k_rs_lds<NL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
    hipLaunchKernelGGL(k_rs_lds<NL>, dim3(b->n_contig), dim3(SW_THREADS), lb, s, *b, *q);
}
