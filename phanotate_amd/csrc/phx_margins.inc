// phx_margins.inc — per-ORF path margins: the out-edge CSR, k_sssp_rev<NL> and k_margins; the re-annotation margins: k_rmg_apply and both under MgCond; the pinned margins: k_pmg_apply and both under MgPin (included by phx_kernels.hip).
// ------------------------------------------------------------------------------------------------
// On demand after a run (phx_margins_flat / phx_tap_dist_target), never inside it.  With d_s the distances the run left in DBatch.dist
// and d_t(v) the exact distance from v TO the target, an ORF edge e = (u -> v) of weight W gets
//     Delta(e) = d_s(u) + W + d_t(v) - D,   D = d_s(target)
// how much longer the best source -> target path becomes when it is forced through e (DESIGN.md §11).
//
// Widths: d_s and d_t are bounded by B, the bound on simple-path sums k_layout2 sized the contig's limb class from (|B| < 2^(64 NL - 5));
// |W| <= B as well (B includes the sum of the ORF weights).  Every partial sum of Delta is therefore below 4 B < 2^(64 NL - 3) in
// magnitude: the contig's own NL limbs hold Delta in two's complement without an extra limb.

// the contigs the pass covers: a graph, no error, distances on the device (sssp_mode 4: solved on the host, no device distances)
__device__ __forceinline__ bool mg_contig(const DMeta *m) { return m->status >= 0 && m->n_node > 2 && m->sssp_mode != 4; }

// ---- the out-edge CSR (transpose of in_off / esrc): count, scan, fill ----
// out_off has V + 1 entries per contig at node_off + contig, like in_off; out-edge records (head node, encoded weight) at edge_off.
// The host zeroes out_off first.  The fill takes slots from the top of a node's range down (atomicSub on the inclusive sums), so that
// out_off ends as exclusive offsets without a second array; the order inside a node's range is whatever the atomics give (the pass
// asks for values only).
__global__ __launch_bounds__(NT) void k_mg_count(DBatch b, DMarg g) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!mg_contig(meta)) return;
    const int V = meta->n_node;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    uint32_t *oo = g.out_off + meta->node_off + blockIdx.x;
    for (int v = (int)blockIdx.y * NT + (int)threadIdx.x; v < V; v += (int)gridDim.y * NT)
        for (uint32_t e = in_off[v], e1 = in_off[v + 1]; e < e1; e++) atomicAdd(&oo[ESRC_NODE(esrc[e])], 1u);
}
__global__ __launch_bounds__(NT) void k_mg_scan(DBatch b, DMarg g) {
    __shared__ uint32_t s_scan[NT / 64 + 1];
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!mg_contig(meta)) return;
    const int n = meta->n_node + 1; // (entry V counts nothing: it ends as the total)
    uint32_t *oo = g.out_off + meta->node_off + blockIdx.x;
    const int per = (n + NT - 1) / NT;
    const int a = (int)threadIdx.x * per, z = a + per < n ? a + per : n;
    uint32_t sum = 0;
    for (int v = a; v < z; v++) sum += oo[v];
    uint32_t tot;
    uint32_t acc = block_excl_scan<NT>(sum, s_scan, &tot);
    for (int v = a; v < z; v++) { acc += oo[v]; oo[v] = acc; } // inclusive
}
__global__ __launch_bounds__(NT) void k_mg_fill(DBatch b, DMarg g) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!mg_contig(meta)) return;
    const int V = meta->n_node;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    uint32_t *oo = g.out_off + meta->node_off + blockIdx.x;
    uint32_t *od = g.out_dst + meta->edge_off;
    long long *ow = g.out_w + meta->edge_off;
    for (int v = (int)blockIdx.y * NT + (int)threadIdx.x; v < V; v += (int)gridDim.y * NT)
        for (uint32_t e = in_off[v], e1 = in_off[v + 1]; e < e1; e++) {
            const uint32_t sw = esrc[e];
            const uint32_t k = atomicSub(&oo[ESRC_NODE(sw)], 1u) - 1u;
            od[k] = (uint32_t)v;
            ow[k] = edge_wenc(sw, ew, e, gt); // (a coded gap edge's integer from the contig's gap table: no k_edges_expand launch in front)
        }
}

// ---- k_sssp_rev<NL>: d_t, one workgroup per contig ----
// Sweep order: the target first, then the CDS / tRNA nodes from the right end down, the source last (node ids are position-sorted with
// source = V-2, target = V-1): edges mostly point right, so a reversed sweep meets a node after nearly all of its out-neighbours.  The
// sweep goes in chunks of NT nodes, Jacobi inside a chunk until it is stable, on the chunk's values in LDS (the out-edges that leave the
// chunk are folded in once per visit: nothing outside it changes meanwhile; reads and writes of an iteration are separated by barriers,
// so no thread ever reads a half-written wide integer).  When a node improves, its in-edges (the predecessors, whose values may now improve)
// widen the work: a predecessor later in the sweep order raises the end of this sweep (s_hi), one earlier in it goes to the next sweep's
// range [s_lo_next, s_hi_next].  So the first sweep visits only chunks that the target's distance has reached, and the later ones only
// what the backward (overlap) edges left open; the pass ends when a sweep leaves nothing open.  At that point no edge can shorten any value:
// the fixed point of min-plus relaxation, which is the exact distance vector (the values are lengths of walks to the target throughout).
// No parents, no tie rule: only the values are asked for.  Bounds like k_sssp: a chunk that does not settle in NT + 8 rounds, or more than
// V + 2 sweeps, is a cycle of negative length (DMarg.mstat = 1: the host reports PHX_S_NEGCYCLE for the contig's margins).

// The policy of k_sssp_rev and k_margins is the type of their second argument.  DMarg: the run's graph, the kernels as §11 describes them.
// MgCond (the re-annotation margins, DESIGN.md §21): the graph G' = G_{F,B} of the last re-annotation, restricted to R, the nodes its solve
// reached.  Everything the policy adds sits behind if constexpr (mg_cond<G>): the DMarg instantiations are the code they were without it.
//   k_sssp_rev  `r.ds` holds the re-solve's d_s' (the contig's NL limbs per node); a node outside R is never relaxed and so never gets a
//               value — the reverse counterpart of §16's "an unreached node is never relaxed", which lets the pass settle whenever the
//               forward solve did (a cycle with one node in R lies in R entirely).  Out-edge position e of the batch (edge_off + e, the
//               CSR's own order) is skipped where its bit is set in r.fbit (refused) and weighs W + B where it is set in r.bbit
//               (B = r.bval[edge_off + e], |B| <= 2^52: ew_decode reads it as the plain integer it is).  Values go to r.dist_t, the
//               verdict to r.mstat; the run's dist_t / mstat (shared with §12 / §13) are not touched.  Contigs: r.sel == 1.
//   k_margins   d_s' from r.ds, d_t' from r.dist_t, D' = d_s'(target); the ORF's in-edge slot is tested in DReann.mask (refused: through =
//               0) and, for a contig solved under the bias policy (DReann.mode), carries DReann.bval where its bit is set in DReann.bbit.
//               Contigs: r.sel != 0 whose reverse pass settled (sel 2 — the re-solve found no path —: D' is unreached, every record through = 0).
struct MgCond : DMarg { DReann q; DRmarg r; };
// MgPin (the pinned margins, DESIGN.md §24): MgCond for a contig solved under the required policy (DReann.mode 2 or 4).  Its d_s' has NL + 1
// limbs per node, the top limb minus the count of required edges behind the node (§16); the pass and the records work on WInt<NL + 1>:
//   k_sssp_rev  as under MgCond, and an out-edge position whose bit is set in r.rbit (required) weighs W + B - M, M = 2^(64 NL): one off the
//               top limb.  d_t' goes to r.dist_t at r.dt_stride words per node reserved, NL + 1 used.
//   k_margins   Delta'' = d_s'(u) + W' + d_t'(v) - D' in NL + 1 limbs; lost = the top limb plus the sign bit of limb NL - 1 (rq_count with
//               the sign turned) to r.lost, margin = float(the low NL limbs as the class's two's complement) / 1000.0.  The ORF's in-edge
//               slot is tested in DReann.req as well.
struct MgPin : DMarg { DReann q; DPmarg r; };
template <class G> constexpr bool mg_cond = !std::is_same<G, DMarg>::value;
template <class G> constexpr bool mg_pin = std::is_same<G, MgPin>::value;
__device__ __forceinline__ bool mg_bit(const uint32_t *bits, uint64_t x) { return (bits[x >> 5] >> (x & 31)) & 1u; } // bit x of a bitmap over the batch's edges
__device__ __forceinline__ int mg_node(int i, int V) { return i == 0 ? V - 1 : (i == V - 1 ? V - 2 : V - 2 - i); } // sweep index -> node id
__device__ __forceinline__ int mg_idx(int v, int V) { return v == V - 1 ? 0 : (v == V - 2 ? V - 1 : V - 2 - v); }  // node id -> sweep index
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_sssp_rev(DBatch b, G g) {
    constexpr bool COND = mg_cond<G>, PIN = mg_pin<G>;
    constexpr int WL = NL + (PIN ? 1 : 0); // limbs of a value: one more under MgPin, whose top limb counts the required edges
    __shared__ int s_flag[2];
    __shared__ int s_hi, s_lo_next, s_hi_next;
    __shared__ uint64_t s_d[NT * WL]; // the current chunk's values, by sweep index - c0
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!mg_contig(meta) || meta->sssp_nl != NL) return;
    if constexpr (COND) { if (g.r.sel[blockIdx.x] != 1) return; }
    const int V = meta->n_node, TGT = V - 1;
    const uint32_t *oo = g.out_off + meta->node_off + blockIdx.x;
    const uint32_t *od = g.out_dst + meta->edge_off;
    const long long *ow = g.out_w + meta->edge_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    uint64_t *dt;
    if constexpr (PIN) dt = g.r.dist_t + (size_t)meta->node_off * g.r.dt_stride;
    else if constexpr (COND) dt = g.r.dist_t + (size_t)meta->node_off * b.dist_stride;
    else dt = g.dist_t + (size_t)meta->node_off * b.dist_stride;
    [[maybe_unused]] const uint64_t *ds = nullptr;
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    if constexpr (COND) ds = g.r.ds + (size_t)meta->node_off * g.r.ds_stride;
    const int tid = threadIdx.x;
    for (int v = tid; v < V; v += NT) {
        WInt<WL> d = wi_inf<WL>();
        bool zero = v == TGT;
        if constexpr (COND) zero = zero && !wi_unreached<WL>(wi_load<WL>(ds + (size_t)v * WL)); // (the target outside R: nothing gets a value)
        if (zero) {
#pragma unroll
            for (int i = 0; i < WL; i++) d.v[i] = 0;
        }
        wi_store<WL>(dt + (size_t)v * WL, d);
    }
    if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; s_hi = 0; s_lo_next = V; s_hi_next = -1; }
    __syncthreads();
    int start = 0, sweeps = 0, it = 0;
    bool bad = false;
    for (;;) {
        for (int c0 = (start / NT) * NT; c0 < V && c0 <= s_hi && !bad; c0 += NT) {
            const int i = c0 + tid;
            const int v = i < V ? mg_node(i, V) : -1;
            const bool relax = v >= 0 && v != TGT;
            uint32_t e0 = relax ? oo[v] : 0u, e1 = relax ? oo[v + 1] : 0u;
            // COND: a node outside R never gets a value (it keeps no out-edges here); `special`: some out-edge position in the bitmap words
            // that cover the node's range is refused or biased — only then are the bitmaps read per edge (the refused and biased edges
            // of a re-annotation are a handful per contig, so nearly every node takes the loops as the plain pass has them)
            [[maybe_unused]] bool special = false;
            if constexpr (COND) {
                if (relax && wi_unreached<WL>(wi_load<WL>(ds + (size_t)v * WL))) e1 = e0;
                if (e1 > e0)
                    for (uint64_t x = (ebase + e0) >> 5, x1 = (ebase + e1 - 1) >> 5; x <= x1; x++) special = special || (g.r.fbit[x] | g.r.bbit[x]) != 0u;
                if constexpr (PIN) { // (the required out-edges are a handful as well: the same test covers them)
                    if (e1 > e0)
                        for (uint64_t x = (ebase + e0) >> 5, x1 = (ebase + e1 - 1) >> 5; x <= x1; x++) special = special || g.r.rbit[x] != 0u;
                }
            }
            // nothing outside the chunk changes while it iterates: the out-edges that leave it are folded in once, the ones inside it
            // read the chunk's values from LDS
            WInt<WL> cur = wi_inf<WL>();
            if (v >= 0) cur = wi_load<WL>(dt + (size_t)v * WL);
            WInt<WL> best = cur;
            for (uint32_t e = e0; e < e1; e++) {
                const uint32_t p = (uint32_t)(mg_idx((int)od[e], V) - c0);
                if (p < (uint32_t)NT) continue;
                if constexpr (COND) { if (special && mg_bit(g.r.fbit, ebase + e)) continue; }
                const WInt<WL> dv = wi_load<WL>(dt + (size_t)od[e] * WL);
                if (wi_is_inf<WL>(dv)) continue;
                WInt<WL> cand = wi_add<WL>(dv, ew_decode<WL>(ow[e]));
                if constexpr (COND) { if (special && mg_bit(g.r.bbit, ebase + e)) cand = wi_add<WL>(cand, ew_decode<WL>(g.r.bval[ebase + e])); }
                if constexpr (PIN) { if (special && mg_bit(g.r.rbit, ebase + e)) cand.v[WL - 1] -= 1ull; } // required: W - M, one off the top limb
                if (wi_lt<WL>(cand, best)) best = cand;
            }
            wi_store<WL>(s_d + (size_t)tid * WL, best);
            __syncthreads();
            int inner = 0;
            bool chg = true;
            while (chg) {
                bool improved = false;
                for (uint32_t e = e0; e < e1; e++) {
                    const uint32_t p = (uint32_t)(mg_idx((int)od[e], V) - c0);
                    if (p >= (uint32_t)NT) continue;
                    if constexpr (COND) { if (special && mg_bit(g.r.fbit, ebase + e)) continue; }
                    const WInt<WL> dv = wi_load<WL>(s_d + (size_t)p * WL);
                    if (wi_is_inf<WL>(dv)) continue;
                    WInt<WL> cand = wi_add<WL>(dv, ew_decode<WL>(ow[e]));
                    if constexpr (COND) { if (special && mg_bit(g.r.bbit, ebase + e)) cand = wi_add<WL>(cand, ew_decode<WL>(g.r.bval[ebase + e])); }
                    if constexpr (PIN) { if (special && mg_bit(g.r.rbit, ebase + e)) cand.v[WL - 1] -= 1ull; }
                    if (wi_lt<WL>(cand, best)) { best = cand; improved = true; }
                }
                __syncthreads(); // every read of this iteration is done
                if (improved) { wi_store<WL>(s_d + (size_t)tid * WL, best); s_flag[it & 1] = 1; }
                if (tid == 0) s_flag[(it + 1) & 1] = 0;
                __syncthreads();
                chg = s_flag[it & 1] != 0;
                it++;
                if (++inner > NT + 8) { bad = true; break; } // a chunk of NT nodes settles in <= NT rounds unless a cycle is negative
            }
            if (v >= 0 && !wi_eq<WL>(best, cur)) { // improved: back to global memory, and the predecessors outside the chunk are open again
                wi_store<WL>(dt + (size_t)v * WL, best);
                int lo = V, hl = -1, hr = -1; // before this chunk (next sweep) / behind it (this sweep)
                for (uint32_t e = in_off[v], x1 = in_off[v + 1]; e < x1; e++) {
                    const int p = mg_idx((int)ESRC_NODE(esrc[e]), V);
                    if (p < c0) { lo = p < lo ? p : lo; hl = p > hl ? p : hl; }
                    else if (p >= c0 + NT) hr = p > hr ? p : hr;
                }
                if (hl >= 0) { atomicMin(&s_lo_next, lo); atomicMax(&s_hi_next, hl); }
                if (hr >= 0) atomicMax(&s_hi, hr);
            }
            __syncthreads(); // (the chunk's values are in global memory and s_hi is final before the next chunk looks)
        }
        __syncthreads();
        if (bad || s_lo_next >= V) break;
        start = s_lo_next;
        const int hn = s_hi_next;
        __syncthreads();
        if (tid == 0) { s_hi = hn; s_lo_next = V; s_hi_next = -1; }
        __syncthreads();
        if (++sweeps > V + 2) { bad = true; break; }
    }
    if constexpr (COND) { if (tid == 0 && bad) g.r.mstat[blockIdx.x] = 1; }
    else { if (tid == 0 && bad) g.mstat[blockIdx.x] = 1; }
}

// ---- k_margins: one thread per ORF (its start node, LINK_START) ----
// (wi_neg: phx_certify.inc)
// float(x) as Python computes it: the integer correctly rounded to a double (round half to even); beyond the double range: +-inf
template <int NL>
__device__ __forceinline__ double wi_to_double_rn(WInt<NL> x) {
    const bool neg = (int64_t)x.v[NL - 1] < 0;
    if (neg) x = wi_neg<NL>(x);
    int p = -1; // bit index of the most significant one
#pragma unroll
    for (int i = 0; i < NL; i++)
        if (x.v[i]) p = 64 * i + 63 - __clzll((long long)x.v[i]);
    if (p < 0) return 0.0;
    // the 64 bits from p down (hi64, its bit 63 = bit p of x) and whether anything below them is set
    uint64_t hi64 = 0;
    bool sticky = false;
    const int lo = p - 63;
    if (lo <= 0) hi64 = x.v[0] << (-lo);
    else {
        const int w = lo >> 6, s = lo & 63;
#pragma unroll
        for (int i = 0; i < NL; i++) {
            if (i == w) { hi64 |= x.v[i] >> s; sticky = sticky || (s && (x.v[i] << (64 - s)) != 0); }
            if (i == w + 1 && s) hi64 |= x.v[i] << (64 - s);
            if (i < w) sticky = sticky || x.v[i] != 0;
        }
    }
    uint64_t mant = hi64 >> 11;
    const uint64_t rb = hi64 & 0x7ffull;
    if (rb > 0x400ull || (rb == 0x400ull && (sticky || (mant & 1ull)))) mant++;
    // mant <= 2^53 is exact in a double; ldexp scales exactly (or overflows to inf)
    const double r = ldexp((double)mant, p - 52);
    return neg ? -r : r;
}

template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_margins(DBatch b, G g) {
    constexpr bool COND = mg_cond<G>, PIN = mg_pin<G>;
    constexpr int WL = NL + (PIN ? 1 : 0);
    const DMeta *meta = &b.meta[blockIdx.x];
    if constexpr (COND) { if (!g.r.sel[blockIdx.x] || !mg_contig(meta) || meta->sssp_nl != NL || g.r.mstat[blockIdx.x]) return; }
    else { if (!mg_contig(meta) || meta->sssp_nl != NL || g.mstat[blockIdx.x]) return; }
    const int V = meta->n_node;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const double *oweight = b.oweight + meta->orf_off;
    const DNode *nd = b.node + meta->node_off;
    const uint32_t *in_off = b.in_off + meta->node_off + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint64_t *ds, *dt;
    phx_orf_margin *rec;
    if constexpr (PIN) { ds = g.r.ds + (size_t)meta->node_off * g.r.ds_stride; dt = g.r.dist_t + (size_t)meta->node_off * g.r.dt_stride; rec = g.r.rec + meta->orf_off; }
    else if constexpr (COND) { ds = g.r.ds + (size_t)meta->node_off * g.r.ds_stride; dt = g.r.dist_t + (size_t)meta->node_off * b.dist_stride; rec = g.r.rec + meta->orf_off; }
    else { ds = b.dist + (size_t)meta->node_off * b.dist_stride; dt = g.dist_t + (size_t)meta->node_off * b.dist_stride; rec = g.rec + meta->orf_off; }
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    const WInt<WL> D = wi_load<WL>(ds + (size_t)(V - 1) * WL);
    const bool d_ok = !wi_unreached<WL>(D);
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const DOrf o = orf[k];
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn; // the edge runs start -> stop on the forward strand, stop -> start on the reverse (functions.py:310-316)
        const DNode nu = nd[u], nv = nd[v];
        phx_orf_margin r;
        r.left = nu.pos; r.right = nv.pos + 2; // as emit_genes (locus.py:29-37)
        r.frame = NFRAME(nu.info);
        r.strand = r.frame < 0 ? -1 : 1;
        r.score = oweight[k];
        r.called = 0; // (the host's: the delivered genes may come from the host re-solve)
        r.through = 0;
        r.margin = __builtin_inf();
        // the ORF's edge among the in-edges of its right node, by its source
        uint32_t e = 0xffffffffu;
        for (uint32_t x = in_off[v], x1 = in_off[v + 1]; x < x1; x++)
            if (ESRC_NODE(esrc[x]) == (uint32_t)u) { e = x; break; }
        if constexpr (COND) { if (e != 0xffffffffu && mg_bit(g.q.mask, ebase + e)) e = 0xffffffffu; } // a refused ORF: no path of G' runs through it
        [[maybe_unused]] int32_t lost = 0;
        if (e != 0xffffffffu && d_ok) {
            const WInt<WL> du = wi_load<WL>(ds + (size_t)u * WL), dv = wi_load<WL>(dt + (size_t)v * WL);
            if (!wi_unreached<WL>(du) && !wi_unreached<WL>(dv)) {
                WInt<WL> w = ew_decode<WL>(edge_wenc(esrc[e], ew, e, gt)); // the edge's own integer, not one recomputed from oweight
                if constexpr (COND) { if (biased && mg_bit(g.q.bbit, ebase + e)) w = wi_add<WL>(w, ew_decode<WL>(g.q.bval[ebase + e])); }
                if constexpr (PIN) { if (mg_bit(g.q.req, ebase + e)) w.v[WL - 1] -= 1ull; } // a required ORF: W' = W + B - M
                const WInt<WL> delta = wi_add<WL>(wi_add<WL>(du, w), wi_add<WL>(dv, wi_neg<WL>(D)));
                r.through = 1;
                if constexpr (PIN) { // Delta'' = lost * M + s: the pins the best path through the ORF gives up, and the class's own signed sum
                    lost = (int32_t)(int64_t)(delta.v[WL - 1] + (delta.v[NL - 1] >> 63));
                    WInt<NL> sl;
#pragma unroll
                    for (int i = 0; i < NL; i++) sl.v[i] = delta.v[i];
                    r.margin = wi_to_double_rn<NL>(sl) / 1000.0;
                } else
                r.margin = wi_to_double_rn<NL>(delta) / 1000.0; // one correctly rounded division, as float(delta) / 1000.0
            }
        }
        rec[k] = r;
        if constexpr (PIN) g.r.lost[meta->orf_off + k] = lost;
    }
}

// ---- re-annotation margins (DESIGN.md §21): what k_sssp_rev<NL, MgCond> reads ----
// On demand after phx_reannotate_flat / phx_evidence_flat (phx_remargins_flat), on the context's stream.  The DBatch is the run's (graph and
// layout, read only), DReann what the re-annotation left resident, DRmarg the feature's own buffers.  A thread per ORF of the contigs with
// DRmarg.sel == 1: a refused or biased ORF (DReann.forb / bias, device ORF order) finds its out-edge in the CSR — the graph stage refuses
// parallel edges, so the head v is unique in u's range — and sets that position's bit in fbit or bbit; a bias writes B to the position's
// word.  Refusal wins over a bias, as in k_rs_mask.  An ORF without an edge is ignored.  Every index is checked against the contig's own
// ranges before use.  The CSR itself is only read.
__global__ __launch_bounds__(NT) void k_rmg_apply(DBatch b, DMarg g, DReann q, DRmarg r) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (r.sel[blockIdx.x] != 1 || !mg_contig(meta)) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const uint8_t *forb = q.forb + meta->orf_off;
    const bool biased = re_mode_bias(q.mode[blockIdx.x]);
    const long long *bias = biased ? q.bias + meta->orf_off : nullptr;
    const uint32_t *oo = g.out_off + meta->node_off + blockIdx.x;
    const uint32_t *od = g.out_dst + meta->edge_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const int V = meta->n_node;
    const uint32_t E = (uint32_t)meta->n_edge;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const uint8_t f = forb[k];
        const long long B = biased ? bias[k] : 0ll;
        if (f != 1 && B == 0) continue;
        const DOrf o = orf[k];
        if (o.grp < 0 || o.grp >= meta->n_grp) continue;
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn; // start -> stop on the forward strand, stop -> start on the reverse (functions.py:310-316)
        if (u < 0 || v < 0 || u >= V || v >= V) continue;
        uint32_t x = oo[u], x1 = oo[u + 1];
        if (x1 > E) x1 = E; // (the CSR's own offsets: never beyond the contig's edges)
        for (; x < x1; x++)
            if (od[x] == (uint32_t)v) { // (no such edge: the ORF is ignored)
                if (f == 1) atomicOr(&r.fbit[(ebase + x) >> 5], 1u << ((ebase + x) & 31));
                else { r.bval[ebase + x] = B; atomicOr(&r.bbit[(ebase + x) >> 5], 1u << ((ebase + x) & 31)); }
                break;
            }
    }
}

// ---- pinned margins (DESIGN.md §24): what k_sssp_rev<NL, MgPin> reads ----
// k_rmg_apply for the contigs with DPmarg.sel == 1 (solved again under the required policy, status 0), with code 2 of DReann.forb as well: a
// required ORF sets its out-edge position's bit in rbit, and, as in k_rs_mask, keeps its bias beside it; a refused one sets fbit and nothing
// else.  The same range checks.
__global__ __launch_bounds__(NT) void k_pmg_apply(DBatch b, DMarg g, DReann q, DPmarg r) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (r.sel[blockIdx.x] != 1 || !mg_contig(meta)) return;
    const DOrf *orf = b.orf + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    const int32_t *onode = b.onode + meta->orf_off;
    const uint8_t *forb = q.forb + meta->orf_off;
    const bool biased = re_mode_bias(q.mode[blockIdx.x]);
    const long long *bias = biased ? q.bias + meta->orf_off : nullptr;
    const uint32_t *oo = g.out_off + meta->node_off + blockIdx.x;
    const uint32_t *od = g.out_dst + meta->edge_off;
    const uint64_t ebase = (uint64_t)meta->edge_off;
    const int V = meta->n_node;
    const uint32_t E = (uint32_t)meta->n_edge;
    for (int k = (int)blockIdx.y * NT + (int)threadIdx.x; k < meta->n_orf; k += (int)gridDim.y * NT) {
        const uint8_t f = forb[k];
        const long long B = biased ? bias[k] : 0ll;
        if (f != 1 && f != 2 && B == 0) continue;
        const DOrf o = orf[k];
        if (o.grp < 0 || o.grp >= meta->n_grp) continue;
        const int sn = onode[k], tn = grp[o.grp].node;
        const bool fwd = o.frame > 0;
        const int u = fwd ? sn : tn, v = fwd ? tn : sn; // start -> stop on the forward strand, stop -> start on the reverse (functions.py:310-316)
        if (u < 0 || v < 0 || u >= V || v >= V) continue;
        uint32_t x = oo[u], x1 = oo[u + 1];
        if (x1 > E) x1 = E; // (the CSR's own offsets: never beyond the contig's edges)
        for (; x < x1; x++)
            if (od[x] == (uint32_t)v) { // (no such edge: the ORF is ignored)
                const uint32_t bit = 1u << ((ebase + x) & 31);
                if (f == 1) atomicOr(&r.fbit[(ebase + x) >> 5], bit);
                else {
                    if (f == 2) atomicOr(&r.rbit[(ebase + x) >> 5], bit);
                    if (B != 0) { r.bval[ebase + x] = B; atomicOr(&r.bbit[(ebase + x) >> 5], bit); }
                }
                break;
            }
    }
}
