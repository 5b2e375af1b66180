// phx_sssp.inc — wide integers; k_sssp / k_path (global memory) and k_sssp_lds (workgroup per contig) (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// Exact integers for the path sums: NL little-endian 64-bit limbs, two's complement.
template <int NL>
struct WInt {
    uint64_t v[NL];
};
#define WINF_TOP 0x7fffffffffffffffull
template <int NL>
__device__ __forceinline__ WInt<NL> wi_inf() {
    WInt<NL> r;
#pragma unroll
    for (int i = 0; i < NL - 1; i++) r.v[i] = 0;
    r.v[NL - 1] = WINF_TOP;
    return r;
}
template <int NL>
__device__ __forceinline__ bool wi_is_inf(const WInt<NL> &a) { return a.v[NL - 1] == WINF_TOP; }
// x is integer-valued (result of trunc()); |x| < 2^(64*NL-2) is guaranteed by the caller's choice of NL
template <int NL>
__device__ __forceinline__ WInt<NL> wi_from_double(double x) {
    WInt<NL> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = 0;
    const uint64_t bits = (uint64_t)__double_as_longlong(x);
    const int ef = (int)((bits >> 52) & 0x7ff);
    if (ef != 0) {
        uint64_t m = (bits & 0xfffffffffffffull) | (1ull << 52);
        const int e = ef - 1075; // value = m * 2^e
        if (e <= 0) {
            if (e > -64) r.v[0] = m >> (-e);
        } else {
            const int w = e >> 6, s = e & 63;
#pragma unroll
            for (int i = 0; i < NL; i++) {
                if (i == w) r.v[i] |= m << s;
                if (i == w + 1 && s) r.v[i] |= m >> (64 - s);
            }
        }
        if (bits >> 63) { // negate
            uint64_t c = 1;
#pragma unroll
            for (int i = 0; i < NL; i++) { uint64_t t = ~r.v[i] + c; c = (c && t == 0) ? 1 : 0; r.v[i] = t; }
        }
    }
    return r;
}
// an edge weight as DBatch.ew keeps it (ew_encode, phx_kernels.hip) -> the integer trunc(w * 1000)
template <int NL>
__device__ __forceinline__ WInt<NL> ew_decode(long long x) {
    if (EW_WIDE(x)) return wi_from_double<NL>(__longlong_as_double(x | (1ll << 62)));
    WInt<NL> r;
    r.v[0] = (uint64_t)x;
#pragma unroll
    for (int i = 1; i < NL; i++) r.v[i] = (uint64_t)(x >> 63);
    return r;
}
template <int NL>
__device__ __forceinline__ WInt<NL> wi_add(const WInt<NL> &a, const WInt<NL> &b) {
    WInt<NL> r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        uint64_t s = a.v[i] + b.v[i];
        uint64_t c1 = s < a.v[i];
        uint64_t s2 = s + c;
        uint64_t c2 = s2 < s;
        r.v[i] = s2;
        c = c1 | c2;
    }
    return r;
}
template <int NL>
__device__ __forceinline__ bool wi_lt(const WInt<NL> &a, const WInt<NL> &b) { // signed a < b
    if (a.v[NL - 1] != b.v[NL - 1]) return (int64_t)a.v[NL - 1] < (int64_t)b.v[NL - 1];
#pragma unroll
    for (int i = NL - 2; i >= 0; i--)
        if (a.v[i] != b.v[i]) return a.v[i] < b.v[i];
    return false;
}
template <int NL>
__device__ __forceinline__ bool wi_eq(const WInt<NL> &a, const WInt<NL> &b) {
    bool e = true;
#pragma unroll
    for (int i = 0; i < NL; i++) e = e && a.v[i] == b.v[i];
    return e;
}
template <int NL>
__device__ __forceinline__ WInt<NL> wi_load(const uint64_t *p) {
    WInt<NL> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = p[i];
    return r;
}
template <int NL>
__device__ __forceinline__ void wi_store(uint64_t *p, const WInt<NL> &a) {
#pragma unroll
    for (int i = 0; i < NL; i++) p[i] = a.v[i];
}

// Shortest path source -> target with exact integer weights trunc(w*1000) (edges.py:22; fastpathz keeps
// the integer part).  The graph is not a DAG (SURVEY.md): nodes are relaxed in position order, window by
// window, each window iterated (Jacobi inside the window, so the result is schedule-independent) until it
// is stable, and the sweep over windows is repeated until a whole sweep changes no distance.  The fixed
// point of min-plus relaxation is the unique exact distance vector.  Ties between equal-length paths are
// broken canonically: parent = the tight in-edge with the lowest in-edge index (every node re-evaluates
// all its in-edges in the last, change-free sweep), see DESIGN.md.
#define PE_NONE 0xffffffffu

// genes of the path (phanotate.py:65-76, locus.py:29-37): every second edge, `nthreads` threads
__device__ void emit_genes(const DBatch &b, const DMeta *meta, const int32_t *path, int npairs, size_t g0, int tid, int nthreads) {
    const DNode *nd = b.node + meta->node_off;
    const DOrf *orf = b.orf + meta->orf_off;
    const double *oweight = b.oweight + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    for (int i = tid; i < npairs; i += nthreads) {
        const int a = path[2 * i + 1], bb = path[2 * i + 2];
        DGene g;
        g.left = nd[a].pos;
        g.right = nd[bb].pos + 2; // locus.py:30
        g.frame = NFRAME(nd[a].info);
        g.strand = g.frame < 0 ? -1 : 1;
        double w = 0.0; // Graph.weight, graphs.py:91-96
        const int ta = NTYPE(nd[a].info);
        if (LINK_KIND(nd[a].link) == LINK_TRNA && LINK_KIND(nd[bb].link) == LINK_TRNA) w = -20.0; // the tRNA edge (functions.py:509); g.frame is +-4
        else if (ta == 0 && g.frame > 0 && LINK_KIND(nd[a].link) == LINK_START) {
            const uint32_t k = LINK_IDX(nd[a].link);
            if (grp[orf[k].grp].node == bb) w = oweight[k];
        } else if (ta == 1 && g.frame < 0 && LINK_KIND(nd[bb].link) == LINK_START) {
            const uint32_t k = LINK_IDX(nd[bb].link);
            if (grp[orf[k].grp].node == a) w = oweight[k];
        }
        g.score = w;
        b.genes[g0 + i] = g;
    }
}


// path -> genes (phanotate.py:65-76, locus.py:29-37); pedge[v] = in-edge index (contig-relative) of v's parent
__device__ void emit_path_and_genes(const DBatch &b, DMeta *meta, const uint32_t *pedge, bool target_reached) {
    meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0;
    const int V = meta->n_node;
    const int SRC = V - 2, TGT = V - 1;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    int32_t *path = b.path + meta->node_off;
    if (!target_reached) { meta->status = PHX_S_NOPATH; return; }
    int n = 0;
    for (int v = TGT; v != SRC && n <= V; v = (int)ESRC_NODE(esrc[pedge[v]])) n++;
    if (n > V) { meta->n_path = -1; return; } // lowest-index parents can run in a circle through a zero-length cycle: k_inorder walks the reference's parents instead
    {
        int k = n;
        for (int v = TGT;; v = (int)ESRC_NODE(esrc[pedge[v]])) { path[k--] = v; if (v == SRC || k < 0) break; }
    }
    meta->n_path = n + 1;
    if (!b.genes) return; // phx_solve: the path is all that is asked for
    const int npairs = n / 2; // shortest_path[1:] taken two at a time (file_handling.pairwise)
    const uint32_t g0 = b.gpack ? (uint32_t)(meta->grp_off + meta->tn_off) : atomicAdd(b.gene_total, (uint32_t)npairs);
    meta->gene_off = g0;
    meta->n_genes = npairs;
    emit_genes(b, meta, path, npairs, (size_t)g0, 0, 1);
}

// ---- general kernel: distances in global memory (any V); also serves phx_solve ----
template <int NL>
__global__ __launch_bounds__(NT) void k_sssp(DBatch b) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    __shared__ int s_flag[2];
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (meta->status < 0 || (V <= 2 && !b.ewl) || meta->sssp_nl != NL || meta->sssp_mode != 0) return; // phanotate.py:63: len(graph) > 2 (phx_solve: any graph)
    if (!b.ewl) { expand_contig(b, meta, (int)threadIdx.x, (int)blockDim.x); __syncthreads(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } // (coded gap edges: this kernel reads plain rows)
    const int SRC = V - 2;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const uint64_t *ewl = b.ewl ? b.ewl + (size_t)meta->edge_off * NL : nullptr; // phx_solve: integer weights given as limbs
    uint64_t *dist = b.dist + (size_t)meta->node_off * b.dist_stride;
    uint32_t *pedge = (uint32_t *)(b.parent + meta->node_off);
    const int tid = threadIdx.x;
    for (int v = tid; v < V; v += NT) {
        WInt<NL> d = wi_inf<NL>();
        if (v == SRC) {
#pragma unroll
            for (int i = 0; i < NL; i++) d.v[i] = 0;
        }
        wi_store<NL>(dist + (size_t)v * NL, d);
        pedge[v] = PE_NONE;
    }
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
    __syncthreads();
    const int nchunk = (V + NT - 1) / NT;
    int sweeps = 0, it = 0;
    bool any = true, bad = false;
    while (any && !bad) {
        any = false;
        for (int c = 0; c < nchunk; c++) {
            const int v = c * NT + tid;
            int inner = 0;
            bool chg = true;
            while (chg) {
                bool improved = false, moved = false;
                WInt<NL> best;
                uint32_t be = PE_NONE;
                if (v < V && v != SRC) {
                    best = wi_load<NL>(dist + (size_t)v * NL);
                    be = pedge[v];
                    const uint32_t be0 = be;
                    const uint32_t e0 = in_off[v], e1 = in_off[v + 1];
                    for (uint32_t e = e0; e < e1; e++) {
                        const uint32_t u = ESRC_NODE(esrc[e]);
                        const WInt<NL> du = wi_load<NL>(dist + (size_t)u * NL);
                        if (wi_is_inf<NL>(du)) continue;
                        const WInt<NL> w = ewl ? wi_load<NL>(ewl + (size_t)e * NL) : ew_decode<NL>(ew[e]);
                        const WInt<NL> cand = wi_add<NL>(du, w);
                        if (wi_lt<NL>(cand, best)) { best = cand; be = e; improved = true; }
                        else if (e < be && wi_eq<NL>(cand, best)) be = e;
                    }
                    moved = be != be0;
                }
                __syncthreads(); // every read of this iteration is done
                if (improved || moved) {
                    if (improved) { wi_store<NL>(dist + (size_t)v * NL, best); s_flag[it & 1] = 1; }
                    pedge[v] = be;
                }
                if (tid == 0) s_flag[(it + 1) & 1] = 0;
                __syncthreads();
                chg = s_flag[it & 1] != 0;
                it++;
                any = any || chg;
                if (++inner > NT + 8) { bad = true; break; } // a chunk of NT nodes converges in <= NT rounds unless a cycle is negative
            }
            if (bad) break;
        }
        if (++sweeps > V + 2) bad = true;
    }
    if (tid == 0) {
        meta->sweeps = sweeps;
        meta->sssp_iters = it;
        if (bad) meta->status = PHX_S_NEGCYCLE;
    }
}

template <int NL>
__global__ void k_path(DBatch b) {
    if (b.tot->overflow) return; // a buffer of this run is too small: the host grows it and runs again
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= b.n_contig) return;
    DMeta *meta = &b.meta[c];
    const int V = meta->n_node;
    if (meta->sssp_nl != NL || meta->sssp_mode != 0) return;
    meta->n_genes = 0; meta->n_path = 0; meta->gene_off = 0;
    if (meta->status < 0 || (V <= 2 && !b.ewl)) return; // phanotate.py:63: len(graph) > 2
    const uint64_t *dist = b.dist + (size_t)meta->node_off * b.dist_stride;
    emit_path_and_genes(b, meta, (const uint32_t *)(b.parent + meta->node_off), dist[(size_t)(V - 1) * NL + NL - 1] != WINF_TOP);
}

// ---- fast kernel: distances and the current window's in-edges live in LDS ----
// 1024 threads = 64 nodes x 16 lanes (one DPP row per node).  A window is 32 new nodes plus the nodes of
// the next 500 bp (every connector edge that points backwards spans < 500 bp, functions.py:372), so that
// after the window has converged its first 32 nodes are final in all but pathological cases; the outer
// sweep loop keeps the result exact regardless.  The relaxation tracks distances only; parents are chosen
// once at the end (lowest-index tight in-edge), which is also what makes ties schedule-independent.
#define SW_ADV 32
#define SW_MAX 64
#ifndef SW_ECAP
#define SW_ECAP 1024
#endif
#ifndef SW_LPN
#define SW_LPN 8 // lanes per node (4, 8 or 16; a DPP row has 16 lanes)
#endif
#define SW_THREADS (SW_MAX * SW_LPN)
//#define SW_PROFILE 1

// "infinity" that survives one addition of any edge weight without wrapping: 2^(64*NL-2).
// Real distances stay below 2^(64*NL-3) in magnitude (the host picks NL that way).
#define WBIG_TOP 0x4000000000000000ull
template <int NL>
__device__ __forceinline__ bool wi_unreached(const WInt<NL> &a) { return (int64_t)a.v[NL - 1] >= (int64_t)0x2000000000000000ull; }
// branch-free signed a < b
template <int NL>
__device__ __forceinline__ bool wi_lt_bf(const WInt<NL> &a, const WInt<NL> &b) {
    bool lt = a.v[0] < b.v[0];
#pragma unroll
    for (int i = 1; i < NL - 1; i++) lt = (a.v[i] < b.v[i]) | ((a.v[i] == b.v[i]) & lt);
    if (NL > 1) lt = ((int64_t)a.v[NL - 1] < (int64_t)b.v[NL - 1]) | ((a.v[NL - 1] == b.v[NL - 1]) & lt);
    return lt;
}
template <int NL>
__device__ __forceinline__ WInt<NL> wi_min_bf(const WInt<NL> &a, const WInt<NL> &b) {
    const bool lt = wi_lt_bf<NL>(b, a);
    WInt<NL> r;
#pragma unroll
    for (int i = 0; i < NL; i++) r.v[i] = lt ? b.v[i] : a.v[i];
    return r;
}
template <int N, int NL>
__device__ __forceinline__ WInt<NL> wi_row_shr(const WInt<NL> &a) {
    WInt<NL> r;
#pragma unroll
    for (int i = 0; i < NL; i++) {
        const uint32_t lo = dpp_row_shr<N>((uint32_t)a.v[i]), hi = dpp_row_shr<N>((uint32_t)(a.v[i] >> 32));
        r.v[i] = ((uint64_t)hi << 32) | lo;
    }
    return r;
}
// after this, the last lane of every SW_LPN-lane group holds the minimum of the group
template <int NL>
__device__ __forceinline__ WInt<NL> wi_row_min(WInt<NL> x, int sub) {
    WInt<NL> y;
    y = wi_min_bf<NL>(x, wi_row_shr<1, NL>(x)); if (sub >= 1) x = y;
    if (SW_LPN > 2) { y = wi_min_bf<NL>(x, wi_row_shr<2, NL>(x)); if (sub >= 2) x = y; }
    if (SW_LPN > 4) { y = wi_min_bf<NL>(x, wi_row_shr<4, NL>(x)); if (sub >= 4) x = y; }
    if (SW_LPN > 8) { y = wi_min_bf<NL>(x, wi_row_shr<8, NL>(x)); if (sub >= 8) x = y; }
    return x;
}
__device__ __forceinline__ uint32_t u32_row_min(uint32_t x, int sub) {
    uint32_t o;
    o = dpp_row_shr<1>(x); if (sub >= 1 && o < x) x = o;
    if (SW_LPN > 2) { o = dpp_row_shr<2>(x); if (sub >= 2 && o < x) x = o; }
    if (SW_LPN > 4) { o = dpp_row_shr<4>(x); if (sub >= 4 && o < x) x = o; }
    if (SW_LPN > 8) { o = dpp_row_shr<8>(x); if (sub >= 8 && o < x) x = o; }
    return x;
}

// Distances of the last SW_RING nodes (node ids are position-sorted, so this is a sliding window over the
// contig) are kept in an LDS ring; every improvement is also written through to the global array, which
// serves the rare reads outside the ring (an ORF edge longer than ~SW_RING nodes, or a backward edge from
// beyond a capped look-ahead).  LDS use is independent of the contig size.
//
// Window k starts at node 32k; its size (32 + look-ahead, <= 64) is planned once per contig.  While window k
// iterates out of LDS, the in-edge tile, the node types, the ring fill-in and the in-edge offsets of window
// k+1 are already in flight into registers, so global-memory latency stays off the critical path.
#ifndef SW_RING
#define SW_RING 1024
#endif
#ifndef SW_RCA
#define SW_RCA 1 // in-edges per lane of a close node kept in registers
#endif
#ifndef SW_RCB
#define SW_RCB 1 // in-edges per lane of an open node kept in registers
#endif
#ifndef SW_WPS
#define SW_WPS 6 // wavefronts per SIMD the register allocation must allow (workgroups/CU = SW_WPS * 256 / SW_THREADS)
#endif
// fixed-size ring of distances + in-edge tile + one plan byte per window of SW_ADV nodes
__host__ __device__ inline size_t sssp_lds_bytes(int V, int nl) {
    return (size_t)(SW_RING + 1) * nl * 8 + (size_t)SW_ECAP * ((size_t)nl * 8 + 4) + (size_t)(V / SW_ADV + 1) + 64;
}
// What differs between the kernels that run the sweep below is its policy P: ring and tile sizes (RING, ECAP) and four switches.
//   SwRun            the run (k_sssp_lds): rows are plain ew[e] (expand_contig has completed them), no mark is ever read, gpack is honoured;
//   ReSw<NL, RePol>  a re-solve (k_rs_lds, k_sc_lds; phx_resolve.inc, which says what the switches mean to the caller): always MASKED.
// MASKED: the rows come through edge_wenc (coded gap edges from the contig's gap table, nothing written to DBatch.ew); an explicit row
// whose bit is set in `mask` (one bit per in-edge slot of the batch) is no edge; the plan lives in LDS up to RS_PLAN_LDS windows, else in
// the caller's `gplan`; gene slots always come from the shared counter.
// REQ: the sweep runs on one limb more than the contig's class, an explicit row whose bit is set in `req` carries W - 2^(64 (NL - 1)) — the
// top limb of a distance is then minus the number of required edges behind it, the limbs below the W-sum (rq_count) —, and a distance that
// counts more than `kreq` required edges ends the solve: only a cycle through a required edge produces one (DESIGN.md §16).
// BIAS: an explicit row whose bit is set in `bbit` carries W + B, B the signed 64-bit word of its in-edge slot in `bval` (read only where
// the bit is set; DESIGN.md §19).  A bonus can make a cycle negative: the sweep and round caps end such a solve, and an unreached node
// stays at the unreached pattern as under REQ.
// REQ and BIAS together (DESIGN.md §22; with BLIST §27): a row weighs W + B - M·[required], on one limb more as under REQ; the count guard and
// the caps are both active.  The tile path then carries three flags per prefetched row — refused and required in r_mk as under REQ, biased
// in a register of its own (r_mb), which no other policy has.
// BLIST (always BIAS): `bval` is not a word per in-edge slot but the solve's own list of (in-edge slot of the batch, B) pairs, sorted by
// in-edge slot, `nbl` of them (DESIGN.md §20); bias_at below is the one place that knows.
struct SwRun { static constexpr int RING = SW_RING, ECAP = SW_ECAP; static constexpr bool MASKED = false, REQ = false, BIAS = false, BLIST = false; };
#define RS_PLAN_LDS 2048 // window-plan bytes kept in LDS (contigs of up to 65 536 nodes); longer plans live in DReann.gplan

// in-edge slot e (source word sw) is refused: coded rows never are (phx_resolve.inc: the bitmap holds bits of explicit rows only)
template <class P>
__device__ __forceinline__ bool rs_refused(const uint32_t *mask, uint64_t ebase, uint32_t sw, uint32_t e) {
    if (!P::MASKED || ESRC_IS_GAP(sw)) return false;
    const uint64_t x = ebase + e;
    return ((mask[x >> 5] >> (x & 31)) & 1u) != 0;
}
// in-edge slot e is required (REQ only; a bit of `req` as one of `mask`, explicit rows only)
template <class P>
__device__ __forceinline__ bool rs_required(const uint32_t *req, uint64_t ebase, uint32_t sw, uint32_t e) {
    if (!P::REQ || ESRC_IS_GAP(sw)) return false;
    const uint64_t x = ebase + e;
    return ((req[x >> 5] >> (x & 31)) & 1u) != 0;
}
// in-edge slot e carries a bias (BIAS only; a bit of `bbit` as one of `mask`, explicit rows only)
template <class P>
__device__ __forceinline__ bool rs_biased(const uint32_t *bbit, uint64_t ebase, uint32_t sw, uint32_t e) {
    if (!P::BIAS || ESRC_IS_GAP(sw)) return false;
    const uint64_t x = ebase + e;
    return ((bbit[x >> 5] >> (x & 31)) & 1u) != 0;
}
// B of in-edge slot x of the batch (edge_off + e), whose bias bit the caller has seen set.  !BLIST: word x of the batch-wide array.  BLIST:
// a binary search of the nbl sorted (in-edge slot, B) pairs at `bval`; a set bit without a pair (the list never lacks one) would read as B = 0.
template <bool BLIST>
__device__ __forceinline__ long long bias_at(const long long *bval, uint64_t x, int nbl) {
    if constexpr (!BLIST) return bval[x];
    else {
        int lo = 0, hi = nbl; // the first pair whose in-edge slot is >= x
        while (lo < hi) { const int mid = (lo + hi) >> 1; if ((uint64_t)bval[2 * mid] < x) lo = mid + 1; else hi = mid; }
        return lo < nbl && (uint64_t)bval[2 * lo] == x ? bval[2 * lo + 1] : 0ll;
    }
}
// required edges counted by a distance of NL limbs under REQ: minus its top limb, less the borrow of a negative W-sum in the limbs below
template <int NL>
__device__ __forceinline__ int64_t rq_count(const WInt<NL> &d) { return -(int64_t)(d.v[NL - 1] + (d.v[NL - 2] >> 63)); }
template <class P>
__device__ __forceinline__ long long sw_row(uint32_t sw, const long long *ew, uint32_t e, const long long *gt) { return P::MASKED ? edge_wenc(sw, ew, e, gt) : ew[e]; }
// the integer of in-edge slot e as the sweep adds it: W, under REQ W - 2^(64 (NL - 1)) for a required row, under BIAS W + B for a biased one
// (|B| <= 2^52, so ew_decode reads it as the plain integer it is)
template <int NL, class P>
__device__ __forceinline__ WInt<NL> sw_weight(uint32_t sw, const long long *ew, uint32_t e, const long long *gt, const uint32_t *req, uint64_t ebase, const uint32_t *bbit = nullptr, const long long *bval = nullptr, const int nbl = 0) {
    if constexpr (!P::REQ && !P::BIAS) return ew_decode<NL>(sw_row<P>(sw, ew, e, gt));
    else {
        WInt<NL> w = ew_decode<NL>(sw_row<P>(sw, ew, e, gt));
        if (rs_required<P>(req, ebase, sw, e)) w.v[NL - 1] -= 1ull;
        if constexpr (P::BIAS) { if (rs_biased<P>(bbit, ebase, sw, e)) w = wi_add<NL>(w, ew_decode<NL>(bias_at<P::BLIST>(bval, ebase + e, nbl))); }
        return w;
    }
}

// The sweep of one contig by one workgroup of SW_THREADS threads (ci: the contig's index in the batch — blockIdx.x where a workgroup is a
// contig; a scenario slot's workgroup passes its slot's contig, phx_resolve.inc): distances to b.dist, lowest-index tight parents to b.parent, then the
// path and the genes.  V = meta->n_node (the caller has read it; after expand_contig's fence a second read would be a second load).
template <int NL, class P>
__device__ __forceinline__ void lds_sweep(const DBatch &b, DMeta *meta, const uint32_t ci, const int V, const uint32_t *mask, uint8_t *gplan, const uint32_t *req = nullptr, const int kreq = 0, const uint32_t *bbit = nullptr, const long long *bval = nullptr, const int nbl = 0) {
    constexpr int RING = P::RING, ECAP = P::ECAP;
    constexpr int EPT = (ECAP + SW_THREADS - 1) / SW_THREADS; // tile edges prefetched per thread
    static_assert(EPT <= 16, "r_mk and r_mb hold 16 flags per field");
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int s_flag[2];
    __shared__ int s_np, s_nclose, s_viol;
    __shared__ uint32_t s_off[2][SW_MAX + 1];
    __shared__ uint8_t s_list[SW_MAX];
    const int tid = threadIdx.x;
    const int SRC = V - 2, TGT = V - 1, ncds = V - 2;
    const uint32_t *in_off = b.in_off + meta->node_off + ci;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = P::MASKED ? gtab_at(b, ci) : nullptr;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const DNode *nd = b.node + meta->node_off;
    uint64_t *gdist = b.dist + (size_t)meta->node_off * b.dist_stride;
    // LDS carve: ring (RING+1)*NL u64 (slot RING = the constant 0 of the source) | tile weights ECAP*NL u64 |
    // tile source slots ECAP u32 | window plan nW bytes.  After convergence the ring+tile area is reused for one
    // parent per node.
    uint64_t *ring = (uint64_t *)smem;
    uint64_t *tw = ring + (size_t)(RING + 1) * NL;
    uint32_t *tsrc = (uint32_t *)(tw + (size_t)ECAP * NL);
    const size_t lds_words = (size_t)(RING + 1) * NL * 2 + (size_t)ECAP * NL * 2 + ECAP; // 32-bit words before the plan
    const int nW = (V + SW_ADV - 1) / SW_ADV;
    uint8_t *plan = !P::MASKED || nW <= RS_PLAN_LDS ? (uint8_t *)(tsrc + ECAP) : gplan + (size_t)(meta->node_off >> 5) + ci; // (a contig's slice: >= V / 32 + 1 bytes)
    for (int v = tid; v < V; v += SW_THREADS) {
        WInt<NL> d;
#pragma unroll
        for (int i = 0; i < NL; i++) d.v[i] = 0;
        if (v != SRC) d.v[NL - 1] = WBIG_TOP;
        wi_store<NL>(gdist + (size_t)v * NL, d);
    }
    if (tid < NL) ring[(size_t)RING * NL + tid] = 0;
#ifdef SW_CENSUS
    if (!P::MASKED && tid == 0) { uint32_t c = atomicAdd(b.gene_total + 1, 1u) + 1; atomicMax(b.gene_total + 2, c); }
#endif
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; }
    // ---- plan: size of every window = SW_ADV nodes to advance by + the nodes of the next 500 bp (<= SW_MAX, tile cap) ----
    for (int k = tid >> 6; k < nW; k += SW_THREADS / 64) {
        const int v0 = k * SW_ADV, lane = tid & 63;
        const int vadv = v0 + SW_ADV < V ? v0 + SW_ADV : V;
        const int idx = v0 + lane;
        bool ok = idx < V;
        if (ok && idx >= vadv) ok = idx < ncds && vadv - 1 < ncds && nd[idx].pos < nd[vadv - 1].pos + 500 && in_off[idx + 1] - in_off[v0] <= (uint32_t)ECAP;
        const uint64_t m = __ballot(ok);
        const int cnt = m == ~0ull ? 64 : __ffsll((long long)~m) - 1;
        if (lane == 0) plan[k] = (uint8_t)cnt; // >= vadv - v0 >= 1
    }
    __syncthreads();
    const int node_l = tid / SW_LPN, sub = tid % SW_LPN;
#ifdef SW_PROFILE
    long long t_setup = 0, t_iter = 0, t_mark = wall_clock64();
#endif
    int sweeps = 0, it = 0;
    bool again = true, bad = false;
    uint32_t *gpe = (uint32_t *)(b.parent + meta->node_off);
    const bool ps_lds = (size_t)V <= lds_words; // else (very large contigs) the final walk chases parent edges in global memory
    uint32_t *psrc = (uint32_t *)smem;
    WInt<NL> big; // the unreached pattern
#pragma unroll
    for (int i = 0; i < NL; i++) big.v[i] = 0;
    big.v[NL - 1] = WBIG_TOP;
    while (again && !bad) {
        int loaded = 0; // nodes [max(0, loaded - RING), loaded) are in the ring
        if (tid < NL) ring[(size_t)RING * NL + tid] = 0; // the constant-zero slot (the LDS is reused by the pass below)
        if (tid == 0) s_viol = 0;
        __syncthreads();
        // registers that carry window k+1's data while window k iterates; bit j of r_mk: tile edge j of this thread is refused, bit 16 + j: required (REQ) or biased (BIAS
        // alone); under REQ and BIAS together (with or without BLIST) bit 16 + j is the required flag and bit j of r_mb the biased one
        uint32_t r_src[EPT];
        long long r_w[EPT];
        uint32_t r_mk = 0;
        [[maybe_unused]] uint32_t r_mb = 0;
        uint32_t r_offn = 0;
        int r_type = 0;
        WInt<NL> r_ring;
        // prologue: window 0.  (The tile loop is written out here and in the window loop: shared through a call or a lambda it costs
        // two VGPRs in the 256-bit class of both kernels and 8 bytes of scratch in k_rs_lds<17>.)
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
                r_w[j] = on ? sw_row<P>(sw, ew, e0n + i, gt) : 0ll;
                if (on && rs_refused<P>(mask, ebase, sw, e0n + i)) r_mk |= 1u << j;
                if (P::REQ && on && rs_required<P>(req, ebase, sw, e0n + i)) r_mk |= 0x10000u << j;
                if constexpr (P::REQ && P::BIAS) { if (on && rs_biased<P>(bbit, ebase, sw, e0n + i)) r_mb |= 1u << j; }
                else if (P::BIAS && on && rs_biased<P>(bbit, ebase, sw, e0n + i)) r_mk |= 0x10000u << j;
            }
        }
        for (int k = 0; k < nW && !bad; k++) {
            const int cur = k & 1;
            const int v0 = k * SW_ADV;
            const int nwin = plan[k];
            const int v1 = v0 + nwin;
            // MASKED (the plan may be in global memory): the next two sizes are read once, here; else where they are used
            const int nwn1 = P::MASKED && k + 1 < nW ? plan[k + 1] : 0, nwn2 = P::MASKED && k + 2 < nW ? plan[k + 2] : 0;
            // ---- commit the prefetched registers of this window to LDS ----
            if (k + 1 < nW && tid <= (P::MASKED ? nwn1 : plan[k + 1])) s_off[cur ^ 1][tid] = r_offn;
            if (tid < 64) { // split the window into close nodes (ORF-edge targets) and open nodes (connector targets)
                const int t = NTYPE(r_type), f = NFRAME(r_type);
                const bool isclose = tid < nwin && ((t == 1 && f > 0) || (t == 0 && f < 0));
                const uint64_t mc = __ballot(isclose);
                const uint64_t mo = __ballot(tid < nwin && !isclose);
                const uint64_t below = tid ? (~0ull >> (64 - tid)) : 0ull;
                const int nc = __popcll(mc);
                if (tid < nwin) s_list[isclose ? __popcll(mc & below) : nc + __popcll(mo & below)] = (uint8_t)tid;
                if (tid == 0) s_nclose = nc;
            }
            // nodes that enter the ring with this window bring their current distance from global memory
            if (loaded + tid < v1) wi_store<NL>(ring + (size_t)((loaded + tid) & (RING - 1)) * NL, r_ring);
            loaded = v1 > loaded ? v1 : loaded;
            const uint32_t e0 = s_off[cur][0];
            const int ne = (int)(s_off[cur][nwin] - e0);
            const bool tiled = ne <= ECAP; // false only if the SW_ADV advance nodes alone exceed the tile
            if (tiled) {
#pragma unroll
                for (int j = 0; j < EPT; j++) {
                    const int i = tid + j * SW_THREADS;
                    if (i < ne) {
                        const uint32_t u = r_src[j];
                        WInt<NL> w = ew_decode<NL>(r_w[j]);
                        // source slot: a ring slot, or the constant-zero slot (the source node; and sources outside the
                        // ring, whose distance cannot change while this window iterates and is folded into the weight)
                        uint32_t sl = RING;
                        if constexpr (P::REQ && P::BIAS) { // both: B first, then the top limb (W + B - M); under BLIST the block below adds B
                            if constexpr (!P::BLIST) { if ((r_mb >> j) & 1u) w = wi_add<NL>(w, ew_decode<NL>(bias_at<false>(bval, ebase + e0 + i, nbl))); }
                            if ((r_mk >> (16 + j)) & 1u) w.v[NL - 1] -= 1ull;
                        } else {
                            if (P::REQ && ((r_mk >> (16 + j)) & 1u)) w.v[NL - 1] -= 1ull; // required: W - M, so the phases pay nothing for it either
                            if constexpr (P::BIAS && !P::BLIST) { if ((r_mk >> (16 + j)) & 1u) w = wi_add<NL>(w, ew_decode<NL>(bias_at<false>(bval, ebase + e0 + i, nbl))); } // biased: W + B, likewise
                        }
                        if (P::MASKED && ((r_mk >> j) & 1u)) w = big; // refused: no edge (0 + "unreached" never wins), so the phases pay nothing for the mask
                        else if (u != (uint32_t)SRC) {
                            if ((int)u < loaded && (int)u + RING >= loaded) sl = u & (RING - 1);
                            else w = wi_add<NL>(w, wi_load<NL>(gdist + (size_t)u * NL));
                        }
                        tsrc[i] = sl;
                        wi_store<NL>(tw + (size_t)i * NL, w);
                    }
                }
                // BLIST: B comes from a search of the slot's list, kept out of the unrolled loop above and done here, where the
                // prefetched rows are no longer live — a thread with a biased row in its part of the tile (rare: a scenario biases
                // a few ORFs) adds B to the entry it has just written; a refused row stays no edge
                // (the biased flags: bits 16.. of r_mk, or r_mb under REQ, where those bits are the required flags — the entry then holds
                // W - M on SNL limbs and takes B second; addition is modular, so that is §22's W + B - M; DESIGN.md §27)
                if constexpr (P::BLIST) {
                    if (P::REQ ? r_mb : r_mk >> 16) {
#pragma nounroll
                        for (int j = 0; j < EPT; j++) {
                            const int i = tid + j * SW_THREADS;
                            if (i < ne && (((P::REQ ? r_mb >> j : r_mk >> (16 + j))) & 1u) && !((r_mk >> j) & 1u))
                                wi_store<NL>(tw + (size_t)i * NL, wi_add<NL>(wi_load<NL>(tw + (size_t)i * NL), ew_decode<NL>(bias_at<true>(bval, ebase + e0 + i, nbl))));
                        }
                    }
                }
            }
            __syncthreads();
            // ---- put window k+1 in flight ----
            if (k + 1 < nW) {
                const int v0n = v0 + SW_ADV, nwn = P::MASKED ? nwn1 : plan[k + 1], v1n = v0n + nwn;
                const uint32_t e0n = s_off[cur ^ 1][0];
                const int nen = (int)(s_off[cur ^ 1][nwn] - e0n);
                r_type = tid < nwn ? nd[v0n + tid].info : 0;
                r_ring = wi_load<NL>(gdist + (size_t)(loaded + tid < v1n ? loaded + tid : 0) * NL);
                r_offn = (k + 2 < nW && tid <= (P::MASKED ? nwn2 : plan[k + 2])) ? in_off[v0n + SW_ADV + tid] : 0u;
                r_mk = 0;
                if constexpr (P::REQ && P::BIAS) r_mb = 0;
#pragma unroll
                for (int j = 0; j < EPT; j++) {
                    const int i = tid + j * SW_THREADS;
                    const bool on = nen <= ECAP && i < nen;
                    const uint32_t sw = on ? esrc[e0n + i] : 0u;
                    r_src[j] = ESRC_NODE(sw);
                    r_w[j] = on ? sw_row<P>(sw, ew, e0n + i, gt) : 0ll;
                    if (on && rs_refused<P>(mask, ebase, sw, e0n + i)) r_mk |= 1u << j;
                    if (P::REQ && on && rs_required<P>(req, ebase, sw, e0n + i)) r_mk |= 0x10000u << j;
                    if constexpr (P::REQ && P::BIAS) { if (on && rs_biased<P>(bbit, ebase, sw, e0n + i)) r_mb |= 1u << j; }
                    else if (P::BIAS && on && rs_biased<P>(bbit, ebase, sw, e0n + i)) r_mk |= 0x10000u << j;
                }
            }
#ifdef SW_PROFILE
            { long long t = wall_clock64(); t_setup += t - t_mark; t_mark = t; }
#endif
            // ---- iterate the window to its fixed point ----
            // The graph is bipartite: close nodes (forward stops, reverse starts) are reached by ORF edges from open
            // nodes only; open nodes (forward starts, reverse stops, target) by connector edges from close nodes and the
            // source only.  One round = phase A (all close nodes) then phase B (all open nodes): inside a phase nobody
            // reads what anybody writes, so results are written at once, and a round advances two hops.
            const int nclose = s_nclose, nopen = nwin - nclose;
            const bool actA = node_l < nclose, actB = node_l < nopen;
            const int lA = actA ? s_list[node_l] : 0, lB = actB ? s_list[nclose + node_l] : 0;
            const int iaA = actA ? (int)(s_off[cur][lA] - e0) + sub : 0, ibA = actA ? (int)(s_off[cur][lA + 1] - e0) : 0;
            const int iaB = actB ? (int)(s_off[cur][lB] - e0) + sub : 0, ibB = actB ? (int)(s_off[cur][lB + 1] - e0) : 0;
            uint64_t *slotA = ring + (size_t)((v0 + lA) & (RING - 1)) * NL, *slotB = ring + (size_t)((v0 + lB) & (RING - 1)) * NL;
            uint64_t *gA = gdist + (size_t)(v0 + lA) * NL, *gB = gdist + (size_t)(v0 + lB) * NL;
            // the first SW_RCA / SW_RCB in-edges of this lane stay in registers for all rounds of the window
            // (close nodes have 1-2 in-edges — the starts of one stop-group; open nodes ~14 — the connectors)
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
            // A phase that changes nothing ends the window: the next phase would read exactly what it read last time.
            // (Exception: the window's very first phase A — phase B has not seen this window's close nodes yet.)
            int inner = 0;
            for (int ph = 0;; ph ^= 1) {
                const bool act = ph ? actB : actA;
                // node groups are compacted per phase: a wavefront whose first group is already past the phase's node
                // count has nothing to do and goes straight to the barrier (wave-uniform branch)
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
                        // the rare rest comes from the LDS tile; the source slot of the next edge is already on its way
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
                            if (rs_refused<P>(mask, ebase, sw, e0 + i)) continue;
                            const uint32_t u = ESRC_NODE(sw);
                            WInt<NL> du;
                            if (u == (uint32_t)SRC) du = wi_load<NL>(ring + (size_t)RING * NL);
                            else if ((int)u < loaded && (int)u + RING >= loaded) du = wi_load<NL>(ring + (size_t)(u & (RING - 1)) * NL);
                            else du = wi_load<NL>(gdist + (size_t)u * NL);
                            best = wi_min_bf<NL>(best, wi_add<NL>(du, sw_weight<NL, P>(sw, ew, e0 + i, gt, req, ebase, bbit, bval, nbl)));
                        }
                    }
                    best = wi_row_min<NL>(best, sub);
                    // (REQ: an unreached node stays at the unreached pattern — relaxed among themselves, the nodes of a cycle through a required
                    // edge that no path from the source reaches would go down by M a turn for ever; such a cycle is no cycle of the solve)
                    // (BIAS: the same for a cycle that a bonus has made negative and the source does not reach — it is no cycle of the solve either)
                    if (act && sub == SW_LPN - 1 && wi_lt_bf<NL>(best, d0) && !((P::REQ || P::BIAS) && wi_unreached<NL>(best))) {
                        wi_store<NL>(myslot, best);
                        wi_store<NL>(ph ? gB : gA, best); // write-through
                        s_flag[it & 1] = 1;
                        if (P::REQ && rq_count<NL>(best) > (int64_t)kreq) s_viol = 2; // more required edges than there are: a cycle through one
                    }
                }
                if (tid == 0) s_flag[(it + 1) & 1] = 0;
                __syncthreads();
                const bool chg = s_flag[it & 1] != 0;
                it++;
                if (!chg && (ph == 1 || inner > 0)) break;
                if (++inner > 2 * SW_MAX + 16) { bad = true; break; }
            }
            if (P::REQ && s_viol == 2) bad = true; // (read behind the phase's barrier; the next write is behind the next window's)
#ifdef SW_PROFILE
            { long long t = wall_clock64(); t_iter += t - t_mark; t_mark = t; }
#endif
        }
        if (++sweeps > V + 2) bad = true;
        __syncthreads();
        // ---- verification + parents in one pass over every in-edge (distances from global memory) ----
        // A node that some in-edge could still improve means the sweep missed a backward dependency that reaches
        // beyond a window's look-ahead: sweep again.  Otherwise the distances are the fixed point and every node
        // takes its tight in-edge with the lowest index as parent (canonical tie-break).  A refused edge neither
        // violates the fixed point nor becomes a parent.
        for (int vb = 0; vb < V; vb += SW_MAX) {
            const int v = vb + node_l;
            uint32_t be = PE_NONE;
            bool viol = false;
            if (v < V) {
                const WInt<NL> dv = wi_load<NL>(gdist + (size_t)v * NL);
                const uint32_t e1 = in_off[v + 1];
                for (uint32_t e = in_off[v] + sub; e < e1; e += SW_LPN) {
                    const uint32_t sw = esrc[e];
                    if (rs_refused<P>(mask, ebase, sw, e)) continue;
                    const WInt<NL> cand = wi_add<NL>(wi_load<NL>(gdist + (size_t)ESRC_NODE(sw) * NL), sw_weight<NL, P>(sw, ew, e, gt, req, ebase, bbit, bval, nbl));
                    if (wi_lt_bf<NL>(cand, dv) && !((P::REQ || P::BIAS) && wi_unreached<NL>(cand))) viol = true;
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
    // ---- path (phanotate.py:64-67) and genes (phanotate.py:71-76, locus.py:29-37) ----
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
                np = n / 2; // shortest_path[1:] taken two at a time (file_handling.pairwise)
                meta->n_genes = np;
                meta->gene_off = !P::MASKED && b.gpack ? (uint32_t)(meta->grp_off + meta->tn_off) : atomicAdd(b.gene_total, (uint32_t)np);
            }
        }
        s_np = np;
#ifdef SW_CENSUS
        if (!P::MASKED) atomicSub(b.gene_total + 1, 1u);
#endif
#ifdef SW_PROFILE
        if (!P::MASKED) { long long t = wall_clock64(); meta->pmax[0] = (uint32_t)t_setup; meta->pmin[0] = (uint32_t)t_iter; meta->sssp_why = (int32_t)(t - t_mark); }
#endif
    }
    __syncthreads();
    const int npairs = s_np;
    if (npairs > 0) emit_genes(b, meta, path, npairs, (size_t)meta->gene_off, tid, SW_THREADS);
}

template <int NL>
__global__ __launch_bounds__(SW_THREADS, NL == 2 ? SW_WPS : (NL == 4 ? 4 : 2)) void k_sssp_lds(DBatch b, int mode, int lds_given) { // (wide classes: a few contigs per batch, registers before occupancy)
    if (b.tot->overflow) return;
    DMeta *meta = &b.meta[blockIdx.x];
    const int V = meta->n_node;
    if (meta->status < 0 || V <= 2 || meta->sssp_nl != NL || meta->sssp_mode != mode) return;
    if (sssp_lds_bytes(V, NL) > (size_t)lds_given) return; // launched with less LDS than this contig needs: left unsolved (sweeps == 0), the host launches again
    if (meta->sweeps != 0) return; // solved by an earlier launch of this run (the launch that runs beside the wavefront kernel)
    expand_contig(b, meta, (int)threadIdx.x, (int)blockDim.x); // (coded gap edges: the sweep reads plain rows)
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    lds_sweep<NL, SwRun>(b, meta, blockIdx.x, V, nullptr, nullptr);
}
