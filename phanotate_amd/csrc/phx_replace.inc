// phx_replace.inc — drop replacements: the best path without each called gene (included by phx_kernels.hip, after phx_drop.inc).
// ------------------------------------------------------------------------------------------------
// On demand after the drop margins (phx_drop.inc, built with DDrop.ps / ts so that the one-hop trees T_s / T_t are kept), never inside a run.
// For every gene slot j (the stop node p_j of a CDS pair of P) with a bypass, a witness: a source -> target path of G - p_j of length
// exactly D_{-g} = D + M_j (DESIGN.md §13):
//
//   1. k_rp_pick: the step-3 winner.  A candidate x -> z covers the slots (first(x), last(z)) and is >= every M_j there, so it attains a
//      slot only if it equals the range maximum of M over the slots it covers: one O(1) test per in-edge by a sparse table of the slots'
//      64-bit saturated M_j (an exact compare where both saturate), then the slots of the range that equal it take x << 32 | z by atomicMin.
//   2. k_rp_cross: the slots whose minimum comes from step 4 only (cx < the step-3 minimum): the delta relaxation inside Y_j once more,
//      with the round each delta settled in; the leaving edge y -> z by the smallest (y, z), then the delta chain back from y through tight
//      in-edges from earlier-settled nodes (lowest id) and the seed edge x -> y_0 (lowest x).
//   3. k_rp_walk: the T_s chain from x to P (p_a), the delta chain, the edge, the T_t chain from z to P (p_b); a node on both tree chains
//      closes a loop of length 0 (the walk is as long as D_{-g}, and what remains a path of G - p_j): it is cut at the node nearest p_a.
//      A counting pass (detour length, genes), the host's offsets, a filling pass (detour, removed and added genes, records).
// Tie rule: (cost; a step-3 candidate before a cross candidate; source node id; head node id), contig-local ids: no batch, flag or CSR order
// enters a witness (the layered trees may choose other tight parents).
// The policy of the three kernels is the type of their second argument, as for the k_dp_* kernels (phx_drop.inc).  DMarg: the run's graph and
// path.  MgDrop (the re-annotation replacements, DESIGN.md §30): the graph G' and the path P' of the last re-annotation, the labels and minima
// of its drop margins (a second DDrop set, with its own one-hop trees), the outputs in a second DRepl set.  Every edge loop skips a refused
// slot and adds the bias of a biased one exactly as k_dp_cand / k_dp_cross<NL, MgDrop> do, so the candidates are the same set; a node outside
// R has no label and enters nothing.  k_rp_walk takes the path and its length from the policy and nothing else: a witness walks tree pointers.
// MgPinDrop (the pinned replacements, DESIGN.md §33): the contigs solved under the required policy, the labels, minima and one-hop trees of
// the pinned drop margins (the pd set), the outputs in a third DRepl set.  What dp_pin<G> adds is what it adds in phx_drop.inc: a value of
// pick and cross has WL = NL + 1 limbs (d_s' / d_t' at WL words per node, the delta buffers, the slot minima at dp_stride words per record),
// and dp_w_in / dp_w_out take one off the top limb of a required slot or position, so "cost" is the (lost, s) order of §32 in every compare.
// The sparse table stays 64-bit: wi_sat64 is monotone in that order (lost > 0 saturates), and a saturated key is decided by the exact
// compare at key == DP_SAT.  k_rp_walk reads node ids only and copies the drop record: `lost` stays where k_dp_rec wrote it.

#define RP_CROSS (1ull << 63) // DRepl.win: a cross winner (y << 32 | z)
#define RP_NONE (~0ull)

// the exact minimum of gene slot j (record i) from the drop kernels' results: *s3 the step-3 part (inf: none), the return value min(s3, cx)
// (W limbs per value, `stride` words reserved per record of DDrop.sx / cx: dp_wl / dp_stride of the caller's policy)
template <int W>
__device__ __forceinline__ WInt<W> rp_slot_min(const DDrop &q, size_t stride, size_t no, int64_t r0, int i, int j, WInt<W> *s3) {
    const uint64_t s = q.slot[no + j];
    const WInt<W> a = s == DP_SAT ? wi_load<W>(q.sx + ((size_t)r0 + i) * stride) : (s == DP_NONE ? wi_inf<W>() : wi_from_u64<W>(s));
    const WInt<W> c = wi_load<W>(q.cx + ((size_t)r0 + i) * stride);
    *s3 = a;
    return wi_lt<W>(c, a) ? c : a;
}

__device__ __forceinline__ void st_l2(uint64_t *p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- 1. k_rp_pick<NL>: the step-3 winners, one workgroup per contig ----
// Level 0 of the table holds M_j saturated to 64 bits at gene slots (DP_NONE: no bypass, which no candidate can cover) and 0 elsewhere
// (never above a candidate); level k entry i the maximum of slots [i, i + 2^k).  In LDS up to DP_TAB_LDS entries, else the contig's slice of
// DDrop.gtab (k_dp_cand is done with it).
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_rp_pick(DBatch b, G g, DDrop q, DRepl r) {
    constexpr bool COND = mg_cond<G>;
    constexpr int WL = dp_wl<NL, G>;
    __shared__ unsigned long long s_tab[DP_TAB_LDS];
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int V = meta->n_node, n = dp_npath<G>(b, g, meta), np = (n - 1) / 2, tid = threadIdx.x;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    const int32_t *first = q.first + no, *last = q.last + no;
    const int64_t r0 = q.roff[blockIdx.x];
    int lv = 1;
    while ((2 << (lv - 1)) <= n) lv++;
    const int cells = n * lv;
    uint64_t *tab = cells <= DP_TAB_LDS ? (uint64_t *)s_tab : q.gtab + q.toff[blockIdx.x];
    for (int j = tid; j < n; j += NT) st_l2(&tab[j], 0);
    __syncthreads();
    for (int i = tid; i < np; i += NT) {
        int j, k;
        if (!dp_gene(b, meta, path, i, &j, &k)) continue;
        WInt<WL> s3;
        const WInt<WL> m = rp_slot_min<WL>(q, dp_stride<G>(b, g), no, r0, i, j, &s3);
        st_l2(&tab[j], wi_is_inf<WL>(m) ? DP_NONE : wi_sat64<WL>(m));
    }
    __syncthreads();
    for (int k = 1; k < lv; k++) {
        const int h = 1 << (k - 1);
        for (int i = tid; i + 2 * h <= n; i += NT) {
            const uint64_t x = ld_l2(&tab[(k - 1) * n + i]), y = ld_l2(&tab[(k - 1) * n + i + h]);
            st_l2(&tab[k * n + i], x > y ? x : y);
        }
        __syncthreads();
    }
    const WInt<WL> negD = wi_neg<WL>(wi_load<WL>(ds + (size_t)(V - 1) * WL));
    for (int z = tid; z < V; z += NT) {
        const int lz = last[z];
        if (lz < 2) continue;
        const WInt<WL> tz = wi_add<WL>(wi_load<WL>(dt + (size_t)z * WL), negD);
        [[maybe_unused]] bool sp = false;
        if constexpr (COND) sp = dp_sp_in(g, biased, ebase, in_off[z], in_off[z + 1]);
        for (uint32_t e = in_off[z], e1 = in_off[z + 1]; e < e1; e++) {
            const uint32_t sw = esrc[e];
            const int x = (int)ESRC_NODE(sw);
            const int fx = first[x];
            if (fx < 0 || fx + 1 > lz - 1) continue;
            if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
            const int a = fx + 1, e2 = lz - 1, k = 31 - __clz(e2 - a + 1);
            const WInt<WL> c = wi_add<WL>(wi_add<WL>(wi_load<WL>(ds + (size_t)x * WL), dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt)))), tz);
            const uint64_t key = wi_sat64<WL>(c);
            const uint64_t m1 = ld_l2(&tab[k * n + a]), m2 = ld_l2(&tab[k * n + e2 - (1 << k) + 1]);
            if (key != (m1 > m2 ? m1 : m2)) continue; // not the range maximum: above every slot it covers
            for (int jj = a; jj <= e2; jj++) {
                if (ld_l2(&tab[jj]) != key) continue;
                const int i = (jj - 1) >> 1;
                int j, ko;
                if (!dp_gene(b, meta, path, i, &j, &ko) || j != jj) continue;
                if (key == DP_SAT) { WInt<WL> s3; if (!wi_eq<WL>(rp_slot_min<WL>(q, dp_stride<G>(b, g), no, r0, i, j, &s3), c)) continue; }
                atomicMin((unsigned long long *)&r.win[r0 + i], (unsigned long long)(((uint64_t)x << 32) | (uint32_t)z));
            }
        }
    }
}

// ---- 2. k_rp_cross<NL>: the cross winners, one workgroup per contig ----
// The cross list as k_dp_cross builds it (DDrop.js / jt); per slot whose minimum only step 4 attains, the Jacobi rounds of k_dp_cross with
// DRepl.rnd[p] = the last round that lowered delta(p) (0: the seed).  A node that settled in round r > 0 has a tight in-edge from a node
// that settled before r, so the chain back from y ends at a seed.  The chain goes to DRepl.chain at an atomically reserved offset.
template <int NL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_rp_cross(DBatch b, G g, DDrop q, DRepl r) {
    constexpr bool COND = mg_cond<G>;
    constexpr int WL = dp_wl<NL, G>;
    __shared__ uint64_t s_d[2][DP_CROSS_LDS * WL];
    __shared__ int s_nc, s_chg;
    __shared__ unsigned long long s_key;
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta) || meta->sssp_nl != NL) return;
    const int V = meta->n_node, np = (dp_npath<G>(b, g, meta) - 1) / 2, tid = threadIdx.x;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const uint32_t *in_off = b.in_off + no + blockIdx.x;
    const uint32_t *esrc = b.esrc + meta->edge_off;
    const long long *ew = b.ew + meta->edge_off;
    const long long *gt = gtab_of(b, meta);
    const uint32_t *oo = g.out_off + no + blockIdx.x;
    const uint32_t *od = g.out_dst + meta->edge_off;
    const long long *ow = g.out_w + meta->edge_off;
    const uint64_t *ds = dp_ds<G>(b, g, meta);
    const uint64_t *dt = dp_dt<G>(b, g, meta);
    [[maybe_unused]] const uint64_t ebase = (uint64_t)meta->edge_off;
    [[maybe_unused]] bool biased = false;
    if constexpr (COND) biased = re_mode_bias(g.q.mode[blockIdx.x]);
    const int32_t *first = q.first + no, *last = q.last + no, *pidx = q.pidx + no;
    int32_t *clist = q.js + no, *cpos = q.jt + no, *rnd = r.rnd + no;
    const int64_t r0 = q.roff[blockIdx.x];
    if (tid == 0) s_nc = 0;
    __syncthreads();
    for (int v = tid; v < V; v += NT) {
        const int f = first[v], l = last[v];
        int p = -1;
        if (pidx[v] < 0 && f >= 0 && l >= 0 && l <= f) { p = atomicAdd(&s_nc, 1); clist[p] = v; }
        cpos[v] = p;
    }
    __syncthreads();
    const int nc = s_nc;
    if (!nc) return;
    uint64_t *bufA = nc <= DP_CROSS_LDS ? s_d[0] : q.da + no * dp_stride<G>(b, g), *bufB = nc <= DP_CROSS_LDS ? s_d[1] : q.db + no * dp_stride<G>(b, g);
    const WInt<WL> negD = wi_neg<WL>(wi_load<WL>(ds + (size_t)(V - 1) * WL));
    for (int i = 0; i < np; i++) {
        int j, k;
        if (!dp_gene(b, meta, path, i, &j, &k)) continue; // (uniform over the workgroup)
        WInt<WL> s3;
        const WInt<WL> m = rp_slot_min<WL>(q, dp_stride<G>(b, g), no, r0, i, j, &s3);
        if (wi_is_inf<WL>(m) || !wi_lt<WL>(m, s3)) continue; // a step-3 candidate attains it (or no bypass)
        if (tid == 0) s_key = RP_NONE;
        __syncthreads();
        auto in_y = [&](int y) { return cpos[y] >= 0 && last[y] <= j && j <= first[y]; };
        for (int p = tid; p < nc; p += NT) {
            const int y = clist[p];
            WInt<WL> d = wi_inf<WL>();
            [[maybe_unused]] bool sp = false;
            if constexpr (COND) { if (in_y(y)) sp = dp_sp_in(g, biased, ebase, in_off[y], in_off[y + 1]); }
            if (in_y(y))
                for (uint32_t e = in_off[y], e1 = in_off[y + 1]; e < e1; e++) {
                    const uint32_t sw = esrc[e];
                    const int x = (int)ESRC_NODE(sw);
                    const int fx = first[x];
                    if (fx < 0 || fx >= j) continue;
                    if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                    const WInt<WL> c = wi_add<WL>(wi_load<WL>(ds + (size_t)x * WL), dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt))));
                    if (wi_lt<WL>(c, d)) d = c;
                }
            wi_store<WL>(bufA + (size_t)p * WL, d);
            rnd[p] = 0;
        }
        __syncthreads();
        uint64_t *cur = bufA, *nxt = bufB;
        for (int rr = 1; rr <= nc + 2; rr++) {
            if (tid == 0) s_chg = 0;
            __syncthreads();
            for (int p = tid; p < nc; p += NT) {
                const int y = clist[p];
                WInt<WL> d = wi_load<WL>(cur + (size_t)p * WL);
                [[maybe_unused]] bool sp = false;
                if constexpr (COND) { if (in_y(y)) sp = dp_sp_in(g, biased, ebase, in_off[y], in_off[y + 1]); }
                if (in_y(y))
                    for (uint32_t e = in_off[y], e1 = in_off[y + 1]; e < e1; e++) {
                        const uint32_t sw = esrc[e];
                        const int x = (int)ESRC_NODE(sw);
                        if (!in_y(x)) continue;
                        if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                        const WInt<WL> dx = wi_load<WL>(cur + (size_t)cpos[x] * WL);
                        if (wi_is_inf<WL>(dx)) continue;
                        const WInt<WL> c = wi_add<WL>(dx, dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(edge_wenc(sw, ew, e, gt))));
                        if (wi_lt<WL>(c, d)) { d = c; s_chg = 1; rnd[p] = rr; }
                    }
                wi_store<WL>(nxt + (size_t)p * WL, d);
            }
            __syncthreads();
            uint64_t *t = cur; cur = nxt; nxt = t;
            const bool chg = s_chg != 0;
            __syncthreads();
            if (!chg) break;
        }
        // the leaving edge: the smallest (y, z) of cost M_j
        for (int p = tid; p < nc; p += NT) {
            const int y = clist[p];
            if (!in_y(y)) continue;
            const WInt<WL> d = wi_load<WL>(cur + (size_t)p * WL);
            if (wi_is_inf<WL>(d)) continue;
            [[maybe_unused]] bool sp = false;
            if constexpr (COND) sp = dp_sp_out(g, ebase, oo[y], oo[y + 1]);
            for (uint32_t e = oo[y], e1 = oo[y + 1]; e < e1; e++) {
                const int z = (int)od[e];
                if (last[z] <= j) continue;
                if constexpr (COND) { if (sp && mg_bit(g.r.fbit, ebase + e)) continue; }
                const WInt<WL> c = wi_add<WL>(wi_add<WL>(d, dp_w_out<WL>(g, sp, ebase + e, ew_decode<WL>(ow[e]))), wi_add<WL>(wi_load<WL>(dt + (size_t)z * WL), negD));
                if (wi_eq<WL>(c, m)) atomicMin(&s_key, (unsigned long long)(((uint64_t)y << 32) | (uint32_t)z));
            }
        }
        __syncthreads();
        if (tid == 0) {
            const uint64_t key = s_key;
            if (key != RP_NONE) {
                // back from y: a tight in-edge from an earlier-settled node of Y_j, the lowest id; then the seed edge x -> y_0, the lowest x
                auto step = [&](int v) -> int {
                    const int pv = cpos[v], rv = rnd[pv];
                    const WInt<WL> dv = wi_load<WL>(cur + (size_t)pv * WL);
                    int best = -1;
                    [[maybe_unused]] bool sp = false;
                    if constexpr (COND) sp = dp_sp_in(g, biased, ebase, in_off[v], in_off[v + 1]);
                    for (uint32_t e = in_off[v], e1 = in_off[v + 1]; e < e1; e++) {
                        const uint32_t sw = esrc[e];
                        const int u = (int)ESRC_NODE(sw);
                        if (best >= 0 && u >= best) continue;
                        if constexpr (COND) { if (sp && mg_bit(g.q.mask, ebase + e)) continue; }
                        const long long we = edge_wenc(sw, ew, e, gt);
                        if (rv == 0) {
                            const int fu = first[u];
                            if (fu < 0 || fu >= j) continue;
                            if (wi_eq<WL>(wi_add<WL>(wi_load<WL>(ds + (size_t)u * WL), dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(we))), dv)) best = u;
                        } else {
                            if (!in_y(u) || rnd[cpos[u]] >= rv) continue;
                            const WInt<WL> du = wi_load<WL>(cur + (size_t)cpos[u] * WL);
                            if (!wi_is_inf<WL>(du) && wi_eq<WL>(wi_add<WL>(du, dp_w_in<WL>(g, sp, biased, ebase + e, ew_decode<WL>(we))), dv)) best = u;
                        }
                    }
                    return best;
                };
                const int y = (int)((key >> 32) & 0x7fffffff);
                int cm = 1, v = y;
                while (rnd[cpos[v]] > 0 && cm <= nc) { v = step(v); if (v < 0) break; cm++; }
                const int x0 = v >= 0 ? step(v) : -1;
                if (v < 0 || x0 < 0 || cm > nc) atomicAdd(&r.cnt[1], 1ull); // (cannot happen: the record stays without a winner)
                else {
                    const int64_t off = (int64_t)atomicAdd(&r.cnt[0], (unsigned long long)cm);
                    if (off + cm <= r.ccap) {
                        v = y;
                        for (int c = cm - 1; c >= 0; c--) { r.chain[off + c] = v; if (c) v = step(v); }
                    }
                    r.coff[r0 + i] = off; r.cm[r0 + i] = cm; r.xs[r0 + i] = x0;
                    r.win[r0 + i] = RP_CROSS | key;
                    atomicAdd(&r.cnt[2], 1ull);
                }
            }
        }
        __syncthreads();
    }
}

// ---- 3. k_rp_walk<FILL>: detours, genes and records, one workgroup per contig, a thread per record ----

// the gene of the pair u -> v, by the rule of emit_genes (phx_sssp.inc)
__device__ __forceinline__ phx_gene rp_gene(const DBatch &b, const DMeta *meta, int a, int bb) {
    const DNode *nd = b.node + meta->node_off;
    const DOrf *orf = b.orf + meta->orf_off;
    const double *oweight = b.oweight + meta->orf_off;
    const DGrp *grp = b.grp + meta->grp_off;
    phx_gene g;
    g.left = nd[a].pos;
    g.right = nd[bb].pos + 2;
    g.frame = NFRAME(nd[a].info);
    g.strand = g.frame < 0 ? -1 : 1;
    double w = 0.0;
    const int ta = NTYPE(nd[a].info);
    if (LINK_KIND(nd[a].link) == LINK_TRNA && LINK_KIND(nd[bb].link) == LINK_TRNA) w = -20.0;
    else if (ta == 0 && g.frame > 0 && LINK_KIND(nd[a].link) == LINK_START) {
        const uint32_t k = LINK_IDX(nd[a].link);
        if (grp[orf[k].grp].node == bb) w = oweight[k];
    } else if (ta == 1 && g.frame < 0 && LINK_KIND(nd[bb].link) == LINK_START) {
        const uint32_t k = LINK_IDX(nd[bb].link);
        if (grp[orf[k].grp].node == a) w = oweight[k];
    }
    g.score = w;
    return g;
}

// pairs (2i+1, 2i+2) of a path with lo <= 2i+1 and 2i+2 <= hi: i in [lo / 2, (hi - 2) / 2]
__device__ __forceinline__ int rp_pairs(int lo, int hi) { return hi < 2 ? 0 : max(0, (hi - 2) / 2 - lo / 2 + 1); }

// The walk of one winner: T_s chain of x (Ls nodes off P, then p_a), [delta chain], T_t chain of z (Lt nodes off P, then p_b).  A node on
// both tree chains: the one nearest p_a (the deepest from x) cuts the loop.  Returns m, the detour's length; out != null: the detour;
// *cut: a loop was cut.
__device__ int rp_walk(const int32_t *pidx, const int32_t *ps, const int32_t *ts, const int32_t *last, int x, int z, const int32_t *mid, int nm,
                       int32_t *out, int *pa, int *pb, bool *cut) {
    int Ls = 0, Lt = 0, v = x;
    while (pidx[v] < 0) { Ls++; v = ps[v]; }
    *pa = pidx[v];
    for (v = z; pidx[v] < 0; v = ts[v]) Lt++;
    *pb = pidx[v];
    int dw = -1, tw = -1;
    const int lz = last[z];
    v = x;
    for (int d = 0; d < Ls; d++, v = ps[v]) {
        if (last[v] != lz) continue; // (every node of z's T_t chain carries last(z))
        int u = z;
        for (int t = 0; t < Lt; t++, u = ts[u]) if (u == v) { dw = d; tw = t; break; }
    }
    const int m = dw >= 0 ? (Ls - dw) + (Lt - tw - 1) : Ls + nm + Lt;
    *cut = dw >= 0;
    if (out) {
        const int d0 = dw >= 0 ? dw : 0;
        v = x;
        for (int d = 0; d < Ls; d++, v = ps[v]) if (d >= d0) out[Ls - 1 - d] = v;
        int p = Ls - d0;
        if (dw < 0) for (int c = 0; c < nm; c++) out[p++] = mid[c];
        v = z;
        for (int t = 0; t < Lt; t++, v = ts[v]) if (dw < 0 || t > tw) out[p++] = v;
    }
    return m;
}

template <int FILL, class G = DMarg>
__global__ __launch_bounds__(NT) void k_rp_walk(DBatch b, G g, DDrop q, DRepl r) {
    const DMeta *meta = &b.meta[blockIdx.x];
    if (!dp_on<G>(b, g, meta)) return;
    const int np = (dp_npath<G>(b, g, meta) - 1) / 2;
    const size_t no = (size_t)meta->node_off;
    const int32_t *path = dp_path<G>(b, g, meta);
    const int32_t *pidx = q.pidx + no, *ps = q.ps + no, *ts = q.ts + no, *last = q.last + no;
    const int64_t r0 = q.roff[blockIdx.x];
    for (int i = threadIdx.x; i < np; i += NT) {
        const int64_t ri = r0 + i;
        int j, k;
        const bool gene = dp_gene(b, meta, path, i, &j, &k);
        const uint64_t key = gene ? r.win[ri] : RP_NONE;
        const bool cross = key != RP_NONE && (key & RP_CROSS);
        int a = -1, bb = -1, m = 0;
        bool cut = false;
        const int z = (int)(uint32_t)key, x = cross ? r.xs[ri] : (int)((key >> 32) & 0x7fffffff);
        const int32_t *mid = cross ? r.chain + r.coff[ri] : nullptr;
        const int nm = cross ? r.cm[ri] : 0;
        if (!FILL) {
            if (key != RP_NONE) {
                m = rp_walk(pidx, ps, ts, last, x, z, mid, nm, nullptr, &a, &bb, &cut);
                if (cut) atomicAdd(&r.cnt[4], 1ull);
                else if (cross) atomicAdd(&r.cnt[3], 1ull); // (the delta chain is part of the detour)
            } else if (gene && q.rec[ri].bypass) atomicAdd(&r.cnt[1], 1ull); // (cannot happen)
            r.info[4 * ri] = a; r.info[4 * ri + 1] = bb; r.info[4 * ri + 2] = m;
            r.info[4 * ri + 3] = key != RP_NONE ? rp_pairs(a, bb) + rp_pairs(a, a + m + 1) : 0;
            continue;
        }
        const phx_gene_drop &dr = q.rec[ri];
        phx_gene_repl rec;
        rec.left = dr.left; rec.right = dr.right; rec.strand = dr.strand; rec.frame = dr.frame;
        rec.drop = dr.drop; rec.called = dr.called; rec.bypass = dr.bypass;
        rec.span_left = dr.left; rec.span_right = dr.right; rec.n_removed = 0; rec.n_added = 0;
        rec.gene_off = r.goff[ri];
        if (key != RP_NONE) {
            int32_t *det = r.det + r.doff[ri];
            m = rp_walk(pidx, ps, ts, last, x, z, mid, nm, det, &a, &bb, &cut);
            phx_gene *gout = r.genes + r.goff[ri];
            int sl = 0x7fffffff, sr = -0x7fffffff, ng = 0;
            for (int p = a / 2; 2 * p + 2 <= bb; p++) {
                const phx_gene ge = rp_gene(b, meta, path[2 * p + 1], path[2 * p + 2]);
                gout[ng++] = ge; sl = min(sl, ge.left); sr = max(sr, ge.right);
            }
            rec.n_removed = ng;
            auto at = [&](int qq) { return qq == a ? path[a] : (qq == a + m + 1 ? path[bb] : det[qq - a - 1]); };
            for (int p = a / 2; 2 * p + 2 <= a + m + 1; p++) {
                const phx_gene ge = rp_gene(b, meta, at(2 * p + 1), at(2 * p + 2));
                gout[ng++] = ge; sl = min(sl, ge.left); sr = max(sr, ge.right);
            }
            rec.n_added = ng - rec.n_removed;
            rec.span_left = sl; rec.span_right = sr;
        }
        r.rec[ri] = rec;
    }
}
